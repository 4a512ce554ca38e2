"""FLUX ControlNet on the MI355X HIP engine: `FluxControlNetModel` (the side network) and `FluxControlNetPipelineRewritePrompt`.

[ext] diffusers >= 0.30 `FluxControlNetModel` / `FluxControlNetPipeline` (InstantX FLUX.1-dev-Controlnet-Canny and -Union, Shakker
Union-Pro), so `prompt_embeds` of any length -- the ThinkDiff aligner's tokens -- supply the content and an edge, depth or pose map the
structure.  **Parity unpinned**: diffusers is not installed; the semantics are restated from its published sources
(`controlnet_flux.py`, `transformer_flux.py`, `pipeline_flux_controlnet.py`) and THIS TEXT IS THE CONTRACT the tests check.
Notation: D = heads x 128; the main transformer has L double and Ls single blocks, the ControlNet n_d double and n_s single blocks
(n_d >= 1, n_s >= 0).

`FluxControlNetModel`
- Parameters: the transformer's `x_embedder`, `context_embedder`, `time_text_embed.*`, `transformer_blocks.*` and
  `single_transformer_blocks.*`; no `norm_out`, no `proj_out`; in addition `controlnet_x_embedder` [D, 64], `controlnet_blocks.{i}`
  [D, D] for i < n_d, `controlnet_single_blocks.{i}` [D, D] for i < n_s (weight and bias each) and, when `num_mode` is set ("union"
  checkpoints), `controlnet_mode_embedder.weight` [num_mode, D].  `guidance_embeds` may be false (InstantX).
- Forward `(hidden, controlnet_cond, controlnet_mode, enc, pooled, timestep, img_ids, txt_ids, guidance)`:
  1. `h = x_embedder(hidden) + controlnet_x_embedder(controlnet_cond)`: each Linear rounds to bf16, then the add rounds.
  2. `temb` as in the transformer; `enc = context_embedder(enc)`.
  3. Union only: `enc = cat([controlnet_mode_embedder[mode][None], enc])` and `txt_ids = cat([txt_ids[:1], txt_ids])` -- the text stream
     has T + 1 rows.  A union model called without a mode is an error.
  4. The n_d double blocks run; `block_sample[i]` is the image stream after block i.
  5. The n_s single blocks run over `[text | image]`; `single_sample[i]` is the image rows after block i.
  6. Outputs `controlnet_blocks[i](block_sample[i])` and `controlnet_single_blocks[i](single_sample[i])`, each bf16 [S_img, D].
  7. Then `sample * conditioning_scale`.  The scale is a Python float, so it is an fp32 operand of the bf16 multiply, not rounded to bf16
     first (the convention of td_flux_cfg_step_kernel); the product rounds to bf16.
- Main transformer with residuals: after double block i `hidden = hidden + block_samples[i // ceil(L / n_d)]` (image stream only); after
  single block i the image rows of `hidden` += `single_samples[i // ceil(Ls / n_s)]`, text rows untouched.  Trailing samples the index
  never reaches are unused, as in diffusers; n_s = 0 means no single-block injection.
- On the engine the samples stay UNSCALED in the ControlNet context's arena, and scale, product rounding and add happen in one kernel
  behind every block of the main forward (td_flux_residual_inject_bf16) -- the same three roundings as steps 6 - 7 and the add.

`FluxControlNetPipelineRewritePrompt.__call__` (`control_image`, `controlnet_conditioning_scale`, `control_guidance_start`,
`control_guidance_end`, `control_mode`)
- Control image: preprocessed like img2img's image, VAE-encoded and sampled with an `eps` drawn from `generator` FIRST, before the
  noise (as in flux_control.py), then `(z - shift) * scaling`, packed to [S, 64].  A tensor [B_img, 16, h, w] is taken as latents (packed
  as it is, no encoder pass, no shift / scale, no eps draw).  Sample b takes control image b % B_img.
- Per-step scale, n steps: `keep[i] = 1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end)`,
  `scale_i = controlnet_conditioning_scale * keep[i]`.
- At step i the ControlNet gets the current latents, the same `timestep / 1000`, the same prompt and pooled embeds and `control_mode`,
  and `guidance` only if its own `guidance_embeds` is true; the transformer call then takes the samples.
- A step with `scale_i == 0` contributes zeros (`h + 0` is `h`): here such a step runs neither the ControlNet nor the injection, and a
  call whose scales are all 0 is the plain text-to-image loop on the same latents.
- Images in flight advance through the existing `denoise_multi`: one (transformer fork, ControlNet fork) pair per image.

`FluxMultiControlNetModel(nets)` ([ext] controlnet_flux.py `FluxMultiControlNetModel.forward`, pipeline_flux_controlnet.py), 1 to 4 nets, as
`controlnet=` of the pipeline
- `control_image` is a list of K entries, each whatever the single-net pipeline takes; `control_mode` a list of K (None for a net without a
  mode embedder); `controlnet_conditioning_scale`, `control_guidance_start`, `control_guidance_end` each one number for all nets or a list
  of K.  Net k's table is `scale_k * keep_k[i]` (`controlnet_scale_tables`).  The generator gives the control images their eps net by net in
  list order, then the noise.
- At one step, for the nets k = 0 .. K-1 in list order with scale c_k (a Python float: an fp32 operand of the bf16 multiply):
      s_k[i] = bf16(c_k * sample_k[i]);   acc[i] = s_0[i];   acc[i] = bf16(float(acc[i]) + float(s_k[i]))  for k = 1 .. K-1
      hidden = bf16(float(hidden) + float(acc[idx]))          (image rows, behind double block i / single block i)
  a left fold with one rounding per add, THEN the add to the hidden state -- one kernel launch per block
  (td_flux_residual_inject_multi_bf16), not K launches of the single-net kernel, which would compute bf16(bf16(h + a) + b).
- **Deviation 1, per-net sample index**: each net uses its own rule `idx_k = i // ceil(n_blocks / n_samples_k)`; diffusers zips the nets'
  sample lists and silently truncates when the counts differ (with equal counts the two agree).  A net without single blocks takes no
  part in the single-block sums.
- **Deviation 2, inactive nets are left out**: a net whose scale at the step is 0 is not run and is left out of the fold; diffusers runs it
  and adds `bf16(0 * x)`, which can differ only in the sign of a zero.  A step at which every net's scale is 0 is the plain step.
- The same `FluxControlNetModel` may appear more than once (a union checkpoint under two modes, two control images): each appearance
  runs on its own fork; with images in flight every transformer context is paired with K ControlNet forks.

Refused, not approximated, each naming what was asked: `conditioning_embedding_channels` / `input_hint_block` (the XLabs pixel-hint
form) and with it `controlnet_blocks_repeat`; a raw Python list as `controlnet=` and per-ControlNet lists given with a single
`FluxControlNetModel` (both point at `FluxMultiControlNetModel([...])`); more than 4 nets, lists of the wrong length, a union net without
its mode; everything flux_control.py refuses (`callback_on_step_end`, custom `sigmas`, lists of generators,
`joint_attention_kwargs`); a ControlNet together with reference tokens, or on a channel-conditioned transformer; 8-bit precision setters
and LoRA ON THE CONTROLNET MODEL (the main transformer may be in any mode, and may carry adapters); a transformer whose first-block cache
is enabled (`ValueError`; the engine refuses the same pairing at the forward).
"""
import ctypes
import dataclasses
import math
from typing import List, Optional

import torch

from .. import _hip
from .flux_fill import refuse_unsupported
from .flux_img2img import FluxImg2ImgPipelineRewritePrompt
from .flux_transformer import _OPS, FluxTransformer2DModel, FluxTransformerConfig, effective_scalar
from .flux_vae import DiagonalGaussianDistribution


@dataclasses.dataclass
class FluxControlNetConfig(FluxTransformerConfig):
    """Keys of a [ext] FluxControlNetModel config.json (InstantX Union: num_layers 5, num_single_layers 10, num_mode 10, guidance_embeds false)."""
    num_mode: Optional[int] = None
    conditioning_embedding_channels: Optional[int] = None


def sample_index(i: int, n_blocks: int, n_samples: int) -> int:
    """Which ControlNet sample block i of `n_blocks` takes: `i // ceil(n_blocks / n_samples)` ([ext] transformer_flux.py)."""
    return i // int(math.ceil(n_blocks / n_samples))


def controlnet_keep(n: int, start: float, end: float) -> List[float]:
    """[ext] pipeline_flux_controlnet.py: keep[i] = 1.0 - float(i / n < start or (i + 1) / n > end)."""
    return [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]


def _refuse_config(c: FluxControlNetConfig) -> None:
    if c.conditioning_embedding_channels is not None:
        raise NotImplementedError(f"conditioning_embedding_channels={c.conditioning_embedding_channels}: the pixel-hint form (input_hint_block, and with "
                                  "it controlnet_blocks_repeat) is not built; ControlNets that read VAE latents load")
    if c.latent_channels != c.in_channels:
        raise ValueError(f"a ControlNet reads the latents alone: in_channels = {c.in_channels}, out_channels = {c.out_channels}")
    if c.num_layers < 1:
        raise ValueError(f"a ControlNet needs at least one double block, got num_layers = {c.num_layers}")


class FluxControlNetModel(FluxTransformer2DModel):
    """The side network on the engine: a second model of the same blocks (td_flux_controlnet_create).  Parameters, `fork`,
    `set_timesteps` are the transformer's; it runs in bf16 only."""

    def __init__(self, config: Optional[FluxControlNetConfig] = None, max_img_tokens: int = 4096, max_txt_tokens: int = 512,
                 max_steps: int = 64, device="cuda", **config_kwargs):
        self.config = config or FluxControlNetConfig(**config_kwargs)
        c = self.config
        _refuse_config(c)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _hip.ThinkDiffHipError("FluxControlNetModel runs on the MI355X HIP engine only (device='cuda')")
        self._L = _hip.lib()
        cc = c.to_hip()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(self._L.td_flux_controlnet_create(ctypes.byref(cc), int(c.num_mode or 0), max_img_tokens, max_txt_tokens, max_steps, ctypes.byref(h)))
        self._h = h
        self.max_img_tokens, self.max_txt_tokens, self.max_steps = max_img_tokens, max_txt_tokens, max_steps
        self._n_steps = 0

    @staticmethod
    def config_from_json(raw: dict) -> FluxControlNetConfig:
        """config.json -> FluxControlNetConfig: known keys only; the pixel-hint form is refused by name."""
        fields = {f.name for f in dataclasses.fields(FluxControlNetConfig)}
        c = FluxControlNetConfig(**{k: v for k, v in raw.items() if k in fields})
        _refuse_config(c)
        return c

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "controlnet", **kw):
        """Local directories only: <path>[/<subfolder>]/{config.json, *.safetensors}; a parameter the checkpoint lacks is an error."""
        return super().from_pretrained(path, subfolder=subfolder, **kw)

    @property
    def union(self) -> bool:
        return bool(self.config.num_mode)

    # ---- what the side network does not take ------------------------------------------------------------------
    def set_precision(self, precision: str = "bf16", **kw):
        if str(precision).replace("torch.", "") not in ("bf16", "bfloat16") or kw.get("smoothing") or kw.get("fp8_gemms") is not None:
            raise NotImplementedError(f"set_precision({precision!r}) on a ControlNet model: the side network runs in bf16 only "
                                      "(set the precision on the main transformer)")
        self.precision = "bf16"
        return self

    def set_attention(self, mode: str = "bf16"):
        if mode != "bf16":
            raise NotImplementedError(f"set_attention({mode!r}) on a ControlNet model: the side network runs in bf16 only")
        self.attention = mode
        return self

    def load_lora_adapter(self, *a, **kw):
        raise NotImplementedError("load_lora_adapter on a ControlNet model: adapters on the side network are not built (the main transformer takes them)")

    def attach_controlnet(self, controlnet):
        raise NotImplementedError("attach_controlnet on a ControlNet model: a ControlNet is attached TO a transformer context")

    def forward_step(self, *a, **kw):
        raise NotImplementedError("a ControlNet has no velocity: forward_samples(latents, step) returns its block samples")

    forward = __call__ = forward_step

    # ---- conditioning ------------------------------------------------------------------------------------------------
    def set_condition(self, prompt_embeds, pooled, img_ids, txt_ids=None, control_mode: Optional[int] = None):
        """The transformer's set_condition; a union model (num_mode set) also takes `control_mode`, the row of controlnet_mode_embedder
        that joins the text stream in front of the prompt (T + 1 text rows, first txt id duplicated)."""
        if self.union and control_mode is None:
            raise ValueError(f"this ControlNet is a union model (num_mode = {self.config.num_mode}): control_mode is required")
        if not self.union and control_mode is not None:
            raise ValueError(f"control_mode = {control_mode} on a ControlNet without a mode embedder (num_mode is not set)")
        _hip.check(self._L.td_flux_controlnet_set_mode(self._h, -1 if control_mode is None else int(control_mode)))
        super().set_condition(prompt_embeds, pooled, img_ids, txt_ids)

    def set_control_condition(self, control_latents):
        """The control image of one image: packed, shifted / scaled VAE latents [S_img, in_channels] bf16.  After set_condition, once per
        image; this context's own (forks hold theirs).  controlnet_x_embedder runs here, once."""
        c = self.config
        assert control_latents.dim() == 2 and control_latents.shape == (self._n_img, c.in_channels), \
            f"control_latents must be [S_img, {c.in_channels}] = {(self._n_img, c.in_channels)}, got {tuple(control_latents.shape)}"
        d = control_latents.to(self.device, torch.bfloat16).contiguous()
        _hip.check(self._L.td_flux_controlnet_set_condition(self._h, _hip.ptr(d), _hip.stream_ptr()))
        torch.cuda.current_stream().synchronize()      # `d` may be a temporary

    def forward_samples(self, latents, step: int, conditioning_scale: Optional[float] = None):
        """One ControlNet evaluation at a prepared step -> (block_samples, single_samples), lists of [S_img, D] bf16 tensors: UNSCALED
        (the engine's form) or, with conditioning_scale, `sample * conditioning_scale` as diffusers returns them."""
        assert latents.dtype == torch.bfloat16 and latents.is_contiguous() and latents.shape == (self._n_img, self.config.in_channels)
        _hip.check(self._L.td_flux_controlnet_forward(self._h, _hip.ptr(latents), int(step), _hip.stream_ptr()))
        c = self.config
        outs = []
        for k in range(c.num_layers + c.num_single_layers):
            t = torch.empty(self._n_img, c.inner_dim, dtype=torch.bfloat16, device=latents.device)
            _hip.check(self._L.td_flux_controlnet_read_sample(self._h, k, _hip.ptr(t), _hip.stream_ptr()))
            outs.append(t if conditioning_scale is None else t * float(conditioning_scale))
        return outs[:c.num_layers], outs[c.num_layers:]


MAX_CONTROLNETS = 4      # TD_MAX_CONTROLNETS of include/thinkdiff_hip.h


class FluxMultiControlNetModel:
    """[ext] diffusers `FluxMultiControlNetModel(nets)`: 1 to 4 `FluxControlNetModel`s whose scaled samples are summed, in list order, before
    they meet the transformer's hidden state.  It owns no weights and no engine context: it is the list, and the only way to the multi
    form of `FluxControlNetPipelineRewritePrompt`.  The same model may appear more than once (one union checkpoint under two modes):
    every appearance runs on its own fork."""

    def __init__(self, nets):
        if isinstance(nets, FluxControlNetModel):
            nets = [nets]
        nets = list(nets)
        if not 1 <= len(nets) <= MAX_CONTROLNETS:
            raise ValueError(f"FluxMultiControlNetModel takes 1 to {MAX_CONTROLNETS} ControlNets, got {len(nets)}")
        for k, m in enumerate(nets):
            if not isinstance(m, FluxControlNetModel):
                raise ValueError(f"FluxMultiControlNetModel: entry {k} is a {type(m).__name__}, not a FluxControlNetModel")
        self.nets = nets

    def __len__(self):
        return len(self.nets)

    def __iter__(self):
        return iter(self.nets)

    def __getitem__(self, k):
        return self.nets[k]


_USE_MULTI = "that form goes with controlnet=FluxMultiControlNetModel([...]); with one FluxControlNetModel"


def _one_number(name: str, v) -> float:
    if isinstance(v, (list, tuple)):
        raise NotImplementedError(f"{name} = {v!r}: per-ControlNet lists: {_USE_MULTI} pass one number")
    return float(v)


def _per_net(name: str, v, K: int) -> list:
    """One entry per ControlNet: a list / tuple of exactly K, or one value for all of them."""
    if isinstance(v, (list, tuple)):
        if len(v) != K:
            raise ValueError(f"{name} has {len(v)} entries for {K} ControlNets: pass one per ControlNet, in the order of FluxMultiControlNetModel([...])"
                             + ("" if name in ("control_image", "control_mode") else ", or one number for all"))
        return list(v)
    return [v] * K


def controlnet_scale_tables(n: int, K: int, conditioning_scale=1.0, start=0.0, end=1.0) -> List[List[float]]:
    """[ext] pipeline_flux_controlnet.py with a FluxMultiControlNetModel: net k's table is `scale_k * keep_k[i]`,
    `keep_k[i] = 1.0 - float(i / n < start_k or (i + 1) / n > end_k)`; each argument one number for all nets or a list of K."""
    sc, st, en = (_per_net(nm, v, K) for nm, v in (("controlnet_conditioning_scale", conditioning_scale), ("control_guidance_start", start),
                                                   ("control_guidance_end", end)))
    return [[float(sc[k]) * kp for kp in controlnet_keep(n, float(st[k]), float(en[k]))] for k in range(K)]


class FluxControlNetPipelineRewritePrompt(FluxImg2ImgPipelineRewritePrompt):
    def __init__(self, *args, controlnet=None, **kw):
        super().__init__(*args, **kw)
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError(f"controlnet is a list of {len(controlnet)} ControlNets: a raw list is not taken, wrap it as FluxMultiControlNetModel([...])")
        self.controlnet = controlnet
        self._cn_pool, self._cn_pool_key = [], None

    def _controlnet_contexts(self, n: int):
        """n rows, one per transformer context of `_contexts`, each holding one ControlNet context per net of the list (created once).
        Row 0 holds the models themselves -- except a model's second appearance in the list, which is a fork like every entry of the
        later rows: one context holds one mode, one control condition and one sample arena."""
        nets = list(self.controlnet.nets) if isinstance(self.controlnet, FluxMultiControlNetModel) else [self.controlnet]
        key = tuple(id(m) for m in nets)
        if self._cn_pool_key != key:
            self._cn_pool, self._cn_pool_key = [[m if all(m is not o for o in nets[:k]) else m.fork() for k, m in enumerate(nets)]], key
        while len(self._cn_pool) < n:
            self._cn_pool.append([m.fork() for m in nets])
        return self._cn_pool[:n]

    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, control_image=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 28, guidance_scale: float = 7.0, controlnet_conditioning_scale=1.0, control_guidance_start=0.0,
                 control_guidance_end=1.0, control_mode=None, num_images_per_prompt: int = 1, generator=None, latents=None,
                 prompt_embeds=None, pooled_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
                 max_sequence_length: int = 512, **kw):
        name = type(self).__name__
        refuse_unsupported(name, generator, kw)
        tr, cn = self.transformer, self.controlnet
        if isinstance(cn, (list, tuple)):
            raise NotImplementedError(f"controlnet is a list of {len(cn)} ControlNets: a raw list is not taken, wrap it as FluxMultiControlNetModel([...])")
        multi = isinstance(cn, FluxMultiControlNetModel)
        if not multi and not isinstance(cn, FluxControlNetModel):
            raise ValueError(f"{name} needs controlnet= a FluxControlNetModel or a FluxMultiControlNetModel, got {type(cn).__name__}")
        if multi:
            nets = list(cn.nets)
            K = len(nets)
            if K > MAX_CONTROLNETS:
                raise ValueError(f"{K} ControlNets: FluxMultiControlNetModel takes 1 to {MAX_CONTROLNETS}")
            if control_image is not None and not isinstance(control_image, (list, tuple)):
                raise ValueError(f"control_image must be a list of {K} entries, one per ControlNet of FluxMultiControlNetModel([...]), got {type(control_image).__name__}")
            images = _per_net("control_image", control_image, K) if control_image is not None else None
            if control_mode is not None and not isinstance(control_mode, (list, tuple)):
                raise ValueError(f"control_mode = {control_mode!r} must be a list of {K} entries, one per ControlNet (None for a net without a mode embedder)")
            modes = _per_net("control_mode", control_mode, K)
            scale_l = [float(v) for v in _per_net("controlnet_conditioning_scale", controlnet_conditioning_scale, K)]
            start_l = [float(v) for v in _per_net("control_guidance_start", control_guidance_start, K)]
            end_l = [float(v) for v in _per_net("control_guidance_end", control_guidance_end, K)]
        else:
            nets, K = [cn], 1
            scale_l = [_one_number("controlnet_conditioning_scale", controlnet_conditioning_scale)]
            start_l = [_one_number("control_guidance_start", control_guidance_start)]
            end_l = [_one_number("control_guidance_end", control_guidance_end)]
            if isinstance(control_mode, (list, tuple)):
                raise NotImplementedError(f"control_mode = {control_mode!r}: per-ControlNet lists: {_USE_MULTI} pass one mode")
            if isinstance(control_image, (list, tuple)) and control_image and isinstance(control_image[0], (list, tuple)):
                raise NotImplementedError(f"control_image is a list of lists (one per ControlNet): {_USE_MULTI} pass its images alone")
            images, modes = ([control_image] if control_image is not None else None), [control_mode]
        for k, m in enumerate(nets):
            tag = f"ControlNet {k} of {K}: " if multi else ""
            mode, start, end = modes[k], start_l[k], end_l[k]
            if m.union and mode is None:
                raise ValueError(f"{tag}this ControlNet is a union model (num_mode = {m.config.num_mode}): control_mode is required")
            if not m.union and mode is not None:
                raise ValueError(f"{tag}control_mode = {mode} on a ControlNet without a mode embedder (num_mode is not set)")
            if m.union and not 0 <= int(mode) < m.config.num_mode:
                raise ValueError(f"{tag}control_mode = {mode} outside the {m.config.num_mode} modes of this ControlNet")
            if start > end:
                raise ValueError(f"{tag}control_guidance_start = {start} exceeds control_guidance_end = {end}")
            if start < 0.0 or end > 1.0:
                raise ValueError(f"{tag}control_guidance_start = {start} / control_guidance_end = {end} outside [0, 1]")
        if getattr(tr, "is_cache_enabled", False):
            raise ValueError(f"{name}: the transformer's first-block cache is enabled and a ControlNet adds its samples behind every block (a skipped step "
                             "runs one block): that pairing is not built; call pipe.transformer.disable_cache() first")
        c_lat = 64
        if tr.config.cond_channels:
            raise NotImplementedError(f"a ControlNet on a channel-conditioned transformer (in_channels = {tr.config.in_channels}, out_channels = "
                                      f"{tr.config.latent_channels}) is not built")
        for k, m in enumerate(nets):
            if (tr.config.in_channels, m.config.in_channels) != (c_lat, c_lat) or tr.config.inner_dim != m.config.inner_dim:
                raise ValueError(f"{name}: transformer (in_channels = {tr.config.in_channels}, inner width {tr.config.inner_dim}) and ControlNet"
                                 f"{f' {k}' if multi else ''} (in_channels = {m.config.in_channels}, inner width {m.config.inner_dim}) must agree, with "
                                 f"{c_lat} latent channels")
        height = int(height or self.default_sample_size * self.vae_scale_factor)
        width = int(width or self.default_sample_size * self.vae_scale_factor)
        if height % 16 or width % 16:
            raise ValueError(f"height and width must be multiples of 16, got {height} x {width}")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if images is None:
            raise ValueError("Provide `control_image`.")
        c, h, w = c_lat // 4, height // 8, width // 8
        S_img = (h // 2) * (w // 2)
        as_latents, imgs, n_ctrl = [], [], []
        for k, ci in enumerate(images):
            tag = f"control_image[{k}]: " if multi else ""
            lat_k = isinstance(ci, torch.Tensor) and ci.dim() == 4 and ci.shape[1] == c
            if lat_k:
                if tuple(ci.shape[2:]) != (h, w):
                    raise ValueError(f"{tag}a {c}-channel control_image is taken as latents and must be [B, {c}, h, w] with (h, w) = {(h, w)}, "
                                     f"got {tuple(ci.shape)}")
                imgs.append(None)
                n_ctrl.append(ci.shape[0])
            else:
                if ci is None:
                    raise ValueError(f"{tag}Provide `control_image`.")
                imgs.append(self._image_list(ci, height, width))
                n_ctrl.append(len(imgs[-1]))
            as_latents.append(lat_k)
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        B = prompt_embeds.shape[0] * num_images_per_prompt
        for k in range(K):
            if B % n_ctrl[k]:
                raise ValueError(f"cannot duplicate {n_ctrl[k]} control images{f' of ControlNet {k}' if multi else ''} to the batch of {B} "
                                 "(prompts x num_images_per_prompt)")
        if latents is not None and tuple(latents.shape) != (B, S_img, c_lat):
            raise ValueError(f"latents must be packed [B, S, {c_lat}] = {(B, S_img, c_lat)}, got {tuple(latents.shape)}")
        if not all(as_latents) and self.vae_encoder is None:
            raise _hip.ThinkDiffHipError("no VAE encoder loaded: build the pipeline with vae_encoder= (or from_pipe / from_pretrained)")
        dev = self._execution_device
        # generator order: the control images' eps, net by net in list order, then the noise
        ctrl = []
        for k in range(K):
            if as_latents[k]:
                ctrl.append([_OPS.flux_pack_latents(images[k][i].to(dev, torch.bfloat16).contiguous()) for i in range(n_ctrl[k])])
            else:
                enc = self.vae_encoder
                moments = [enc.encode_moments(im) for im in imgs[k]]
                eps = torch.randn((n_ctrl[k], c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
                dist = DiagonalGaussianDistribution(moments, h, w)
                ctrl.append([dist.packed_latents(i, eps[i], None, 0.0, self.vae_scaling_factor, self.vae_shift_factor) for i in range(n_ctrl[k])])
        lat, _, _ = self.prepare_latents(B, height, width, generator, latents)
        sig = self.scheduler.sigmas(num_inference_steps, S_img)
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_bf = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float())
        g_eff = g_bf if tr.config.guidance_embeds else 0.0
        scales = controlnet_scale_tables(num_inference_steps, K, scale_l, start_l, end_l)
        control = None
        if any(s != 0.0 for tab in scales for s in tab):      # all zero: every step is the plain step -- the text-to-image loop
            control = dict(conds=[[ctrl[k][b % n_ctrl[k]] for k in range(K)] for b in range(B)], scales=scales, modes=modes,
                           g_eff=[g_bf if m.config.guidance_embeds else 0.0 for m in nets])
        xs = self._denoise_controlled(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff, control)
        return self._finish(xs, h, w, output_type, return_dict)

    def _denoise_controlled(self, lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff, control):
        """`_denoise_groups` with the ControlNet contexts of one row of `_controlnet_contexts` attached to every transformer context for the
        duration of the loop: each ControlNet context gets the sample's prompt, pooled embeds, ids, ITS control mode and control latents and the
        same schedule; the main context gets one scale table per net."""
        if control is None:
            return self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff)
        G = max(1, min(int(self.images_in_flight), B))
        ctxs, cns = self._contexts(G), self._controlnet_contexts(G)
        n_prompts = prompt_embeds.shape[0]
        tr = self.transformer
        main = torch.cuda.current_stream()
        xs = []
        try:
            for k in range(G):
                ctxs[k].attach_controlnets(cns[k])
            for b0 in range(0, B, G):
                group = list(range(b0, min(b0 + G, B)))
                lat_g = []
                for k, b in enumerate(group):
                    pb = min(b // num_images_per_prompt, n_prompts - 1)
                    st = self._streams[k]
                    st.wait_stream(main)
                    with torch.cuda.stream(st):
                        pe, po = prompt_embeds[pb], pooled_prompt_embeds[min(pb, pooled_prompt_embeds.shape[0] - 1)]
                        ctxs[k].set_condition(pe, po, img_ids, text_ids)
                        ctxs[k].set_timesteps(t_eff, g_eff)
                        for j, cnj in enumerate(cns[k]):
                            ctxs[k].set_controlnet_scales(control["scales"][j], net=j)
                            cnj.set_condition(pe, po, img_ids, text_ids, control_mode=control["modes"][j])
                            cnj.set_control_condition(control["conds"][b][j])
                            cnj.set_timesteps(t_eff, control["g_eff"][j])
                        lat_g.append(lat[b].contiguous())
                if len(group) == 1:
                    with torch.cuda.stream(self._streams[0]):
                        ctxs[0].denoise(lat_g[0], sig)
                else:
                    type(tr).denoise_multi(ctxs[:len(group)], lat_g, sig, self._streams[:len(group)])
                for k in range(len(group)):
                    main.wait_stream(self._streams[k])
                xs.extend(lat_g)
        finally:
            for k in range(G):      # the transformer's contexts are shared with the other pipelines: leave them plain
                ctxs[k].attach_controlnets([])
        return xs
