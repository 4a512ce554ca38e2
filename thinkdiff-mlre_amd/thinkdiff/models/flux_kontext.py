"""`FluxKontextPipelineRewritePrompt`: FLUX.1 Kontext (in-context image editing) on the MI355X HIP engine.

[ext] diffusers >= 0.34 `FluxKontextPipeline.__call__` (image=, true_cfg_scale=, negative_prompt*=) on top of
`FluxImg2ImgPipelineRewritePrompt`, so `prompt_embeds` of any length -- the ThinkDiff aligner's tokens -- drive an edit that sees the
pixels of the input image in context.  **Parity unpinned**: diffusers is not installed (and the rest of the repository follows 0.31.0,
which has no Kontext pipeline); the semantics are restated from its published source (`pipeline_flux_kontext.py`) and THIS TEXT IS THE
CONTRACT the tests check.  B = prompts x num_images_per_prompt, C = 16; S = (H/16)(W/16) latent tokens of the H x W output,
S_ref = (H_r/16)(W_r/16) reference tokens of the H_r x W_r reference image.

- The transformer is the FLUX.1-dev one (`in_channels == out_channels == 64`).  Every forward runs over
  `[text | latents | reference-image latents]`; only the first S image rows of its output are a velocity.  diffusers does that with a
  `torch.cat` and a slice per step; here the reference tokens are written once per image into the engine context that carries the
  sample (`FluxTransformer2DModel.set_reference_tokens`) and the engine's own loops (`td_flux_denoise` / `_multi` / `_cfg`) run as
  they do for text-to-image.
- Output size: `(height, width)` (default 1024 x 1024) is rescaled to `max_area` at its own aspect ratio `ar = width / height`:
  `width = round(sqrt(max_area * ar))`, `height = round(sqrt(max_area / ar))`, each floored to a multiple of 16; a warning when that
  changes what the caller asked for.
- Reference size: with `_auto_resize` (default) a PIL image goes to the entry of `PREFERRED_KONTEXT_RESOLUTIONS` (width, height)
  whose `w / h` is nearest the image's, ties by the tuple order of `min((abs(ar - w / h), w, h) ...)`; without it the image keeps its
  size (each image of a list by its own size: diffusers sizes a list by its first image).  Either way the size is floored to
  multiples of 16, PIL images are resized on the host (LANCZOS, `_image_list`) and
  preprocessed on the GPU in front of the encoder, as in the image-to-image pipeline.  Float tensors [B_img, 3, H_r, W_r] in [0, 1]
  are NOT resized (`_auto_resize` does not apply to them) and must already have a size that is a multiple of 16.  The reference may
  have another size than the output: S_ref != S in general.  A tensor `image` with 16 channels [B_img, 16, h_r, w_r] is taken as
  the (shifted, scaled) latents as it is and only packed.  The VAE encoder's capacity must hold the reference (all 17 preferred
  sizes need `max_image_size=(1568, 1568)`).
- Reference latents: `latent_dist.mode()` (diffusers' `sample_mode="argmax"`), so NO generator draw; `(z - shift) * scaling`,
  `_pack_latents` -- td_vae_latents_from_moments without eps and without noise.  Sample b takes image `b % B_img`;
  `B % B_img != 0` is an error.
- Ids: latents `(0, y, x)` as everywhere; reference `(1, y, x)` over its own `(H_r/16, W_r/16)` grid.
- Generator order: only the noise `randn([B, 16, h, w], generator, device, bf16)`, skipped when packed `latents` [B, S, 64] are given.
- Schedule: the full text-to-image schedule `sigmas(N, S)`: the shift `mu` comes from the latents' token count, not from S + S_ref.
- True classifier-free guidance is on when `true_cfg_scale > 1` AND a negative prompt was given (`negative_prompt` text, or both
  `negative_prompt_embeds` and `negative_pooled_prompt_embeds`); `true_cfg_scale > 1` without one is a warning and the plain loop,
  and so is a negative prompt with `true_cfg_scale <= 1` (the negative prompt is ignored).
  The negative prompt goes through the same `encode_prompt`; per step both conditionings run over the same latents and reference
  tokens and `noise_pred = neg + true_cfg_scale * (pos - neg)` feeds the Euler step (td_flux_denoise_cfg: one context pair, one
  stream, samples one after another; the fused step is td_flux_cfg_step_bf16).  Without true CFG, `images_in_flight` samples advance
  together as in the other pipelines.
- `image=None` is plain text-to-image on the same loop: `FluxPipelineRewritePrompt`'s output for the same generator.
- Output: `_finish` as in the other pipelines.

Refused, not approximated (NotImplementedError, before any device call): `callback_on_step_end`, custom `sigmas`, lists of
generators, `joint_attention_kwargs` (a LoRA's weight is set with `set_adapters(names, weights)`), the IP-adapter arguments, a list of reference images per sample.  A keyword that is neither in the
call surface nor one of those is a TypeError (a misspelt `negative_prompt` must not run the plain loop silently).  A transformer that is not
64 / 64 is refused with both numbers named; an image stream S + S_ref beyond the transformer's `max_img_tokens` is refused with the
numbers and the constructor argument to raise (the default 4096 holds a 1024 x 1024 output alone; with a 1024 x 1024 reference
Kontext wants 8192).
"""
import warnings
from typing import Optional

import torch

from .. import _hip
from .flux_fill import refuse_unsupported, require_channels
from .flux_img2img import FluxImg2ImgPipelineRewritePrompt
from .flux_transformer import _OPS, effective_scalar
from .flux_vae import DiagonalGaussianDistribution

# (width, height), [ext] pipeline_flux_kontext.py
PREFERRED_KONTEXT_RESOLUTIONS = [
    (672, 1568), (688, 1504), (720, 1456), (752, 1392), (800, 1328), (832, 1248), (880, 1184), (944, 1104), (1024, 1024),
    (1104, 944), (1184, 880), (1248, 832), (1328, 800), (1392, 752), (1456, 720), (1504, 688), (1568, 672)]

IP_ADAPTER_ARGS = ("ip_adapter_image", "ip_adapter_image_embeds", "negative_ip_adapter_image", "negative_ip_adapter_image_embeds")
# keywords diffusers' call has and this one refuses when set (None is accepted); any other unknown keyword is a TypeError, as in Python
REFUSED_ARGS = ("callback_on_step_end", "callback_on_step_end_tensor_inputs", "sigmas", "joint_attention_kwargs") + IP_ADAPTER_ARGS

MULTIPLE_OF = 16      # vae_scale_factor (8) x the 2 x 2 patch


def output_size(height: int, width: int, max_area: int):
    """(height, width) rescaled to max_area at its own aspect ratio, floored to multiples of 16 -> (height, width)."""
    ar = width / height
    w = round((max_area * ar) ** 0.5)
    h = round((max_area / ar) ** 0.5)
    return h // MULTIPLE_OF * MULTIPLE_OF, w // MULTIPLE_OF * MULTIPLE_OF


def reference_size(image_height: int, image_width: int, auto_resize: bool = True):
    """The size the reference image is resized to -> (height, width)."""
    if auto_resize:
        ar = image_width / image_height
        _, image_width, image_height = min((abs(ar - w / h), w, h) for w, h in PREFERRED_KONTEXT_RESOLUTIONS)
    return image_height // MULTIPLE_OF * MULTIPLE_OF, image_width // MULTIPLE_OF * MULTIPLE_OF


def reference_ids(h2: int, w2: int, device=None) -> torch.Tensor:
    """ids of the reference tokens over their own (h2, w2) grid: (1, y, x)."""
    ids = torch.zeros(h2, w2, 3)
    ids[..., 0] = 1
    ids[..., 1] += torch.arange(h2)[:, None]
    ids[..., 2] += torch.arange(w2)[None, :]
    return ids.reshape(h2 * w2, 3).to(device)


class FluxKontextPipelineRewritePrompt(FluxImg2ImgPipelineRewritePrompt):
    def _reference_tokens(self, image, auto_resize: bool):
        """`image` -> per reference image its latent size (h_r, w_r) and a thunk that makes its packed latents [S_ref, 64].  Everything here
        is host-side (sizes, refusals, the PIL resize); the thunks -- the encoder -- run only after every check of the call has passed."""
        from PIL import Image
        dev = self._execution_device
        if isinstance(image, torch.Tensor) and image.dim() == 3:
            image = image[None]
        if isinstance(image, torch.Tensor) and image.dim() == 4 and image.shape[1] == 16:      # latents as they are
            if image.shape[2] % 2 or image.shape[3] % 2:
                raise ValueError(f"latent `image` must have even height and width, got {tuple(image.shape)}")
            hw = [(int(image.shape[2]), int(image.shape[3]))] * image.shape[0]
            make = [lambda i=i: _OPS.flux_pack_latents(image[i].to(dev, torch.bfloat16).contiguous()) for i in range(image.shape[0])]
        else:
            if isinstance(image, torch.Tensor):
                Hr, Wr = int(image.shape[-2]), int(image.shape[-1])
                if Hr % MULTIPLE_OF or Wr % MULTIPLE_OF:
                    raise ValueError(f"image tensor is {(Hr, Wr)}: tensor inputs are not resized and must have a height and width that "
                                     f"are multiples of {MULTIPLE_OF} (resize on the host, or pass PIL images)")
                groups = [(image, Hr, Wr)]
            else:
                pil = list(image) if isinstance(image, (list, tuple)) else [image]
                groups = []
                for im in pil:
                    if isinstance(im, (list, tuple)):
                        raise NotImplementedError("several reference images per sample are not supported: pass one image, or one per sample")
                    if not isinstance(im, Image.Image):
                        raise ValueError(f"image must be a PIL image, a list of them or a float tensor, got {type(im)}")
                    Hr, Wr = reference_size(im.height, im.width, auto_resize)
                    if Hr == 0 or Wr == 0:
                        raise ValueError(f"reference image {im.width} x {im.height} is smaller than {MULTIPLE_OF} pixels")
                    groups.append((im, Hr, Wr))
            enc = self.vae_encoder
            if enc is None:
                raise _hip.ThinkDiffHipError("no VAE encoder loaded: build the pipeline with vae_encoder= (or from_pipe / from_pretrained)")
            cap = enc.max_image_size
            for _, Hr, Wr in groups:
                if Hr * Wr > cap[0] * cap[1]:
                    raise ValueError(f"reference image {Wr} x {Hr} = {Hr * Wr} pixels exceeds the VAE encoder's capacity {cap[0]} x {cap[1]} = "
                                     f"{cap[0] * cap[1]}: build AutoencoderKLEncoder with a larger max_image_size (Kontext's preferred sizes "
                                     f"need max_image_size=(1568, 1568))")
            hw, make = [], []
            for src, Hr, Wr in groups:
                for im in self._image_list(src, Hr, Wr):
                    hw.append((Hr // 8, Wr // 8))
                    make.append(lambda im=im, Hr=Hr, Wr=Wr: DiagonalGaussianDistribution([enc.encode_moments(im)], Hr // 8, Wr // 8).packed_latents(
                        0, None, None, 0.0, self.vae_scaling_factor, self.vae_shift_factor))
        return hw, make

    @torch.no_grad()
    def __call__(self, image=None, prompt=None, prompt_2=None, negative_prompt=None, negative_prompt_2=None, true_cfg_scale: float = 1.0,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 28, guidance_scale: float = 3.5,
                 num_images_per_prompt: int = 1, generator=None, latents=None, prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
                 max_sequence_length: int = 512, max_area: int = 1024 ** 2, _auto_resize: bool = True, **kw):
        name = type(self).__name__
        refuse_unsupported(name, generator, kw)
        for key in IP_ADAPTER_ARGS:
            if kw.get(key) is not None:
                raise NotImplementedError(f"{key} is not supported by {name}")
        unknown = sorted(k for k in kw if k not in REFUSED_ARGS)
        if unknown:
            raise TypeError(f"{name}.__call__() got unexpected keyword arguments {unknown}")
        tr = self.transformer
        c_lat = 64
        require_channels(name, tr.config, c_lat, c_lat)
        height = int(height or self.default_sample_size * self.vae_scale_factor)
        width = int(width or self.default_sample_size * self.vae_scale_factor)
        asked = (height, width)
        height, width = output_size(height, width, int(max_area))
        if (height, width) != asked:
            warnings.warn(f"Generation `height` and `width` have been adjusted to {height} and {width} to fit the model requirements.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        has_neg = negative_prompt is not None or (negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None)
        do_true_cfg = true_cfg_scale > 1 and has_neg
        if true_cfg_scale > 1 and not has_neg:
            warnings.warn(f"true_cfg_scale is passed as {true_cfg_scale}, but classifier-free guidance is not enabled since no negative_prompt is provided.")
        elif true_cfg_scale <= 1 and has_neg:
            warnings.warn("negative_prompt is passed but classifier-free guidance is not enabled since true_cfg_scale <= 1")
        h, w = height // 8, width // 8
        S_img = (h // 2) * (w // 2)
        # reference sizes and every capacity check on the host, before the first device call
        ref_hw, ref_make = ([], []) if image is None else self._reference_tokens(image, bool(_auto_resize))
        for hr, wr in ref_hw:
            S_ref = (hr // 2) * (wr // 2)
            if S_img + S_ref > tr.max_img_tokens:
                raise ValueError(f"{name}: the image stream of {S_img} latent + {S_ref} reference tokens = {S_img + S_ref} exceeds the "
                                 f"transformer's capacity {tr.max_img_tokens}: build FluxTransformer2DModel with max_img_tokens >= {S_img + S_ref} "
                                 f"(a 1024 x 1024 output with a 1024 x 1024 reference wants 8192)")
        if S_img > tr.max_img_tokens:
            raise ValueError(f"{name}: {S_img} latent tokens exceed the transformer's capacity {tr.max_img_tokens} (max_img_tokens)")
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        cfg = None
        if do_true_cfg:
            neg_embeds, neg_pooled, neg_ids = self.encode_prompt(
                prompt=negative_prompt, prompt_2=negative_prompt_2, prompt_embeds=negative_prompt_embeds,
                pooled_prompt_embeds=negative_pooled_prompt_embeds, num_images_per_prompt=num_images_per_prompt,
                max_sequence_length=max_sequence_length)
            cfg = (neg_embeds, neg_pooled, neg_ids, float(true_cfg_scale))
        B = prompt_embeds.shape[0] * num_images_per_prompt
        if ref_hw and B % len(ref_hw):
            raise ValueError(f"Cannot duplicate `image` of batch size {len(ref_hw)} to {B} samples.")
        if latents is not None and tuple(latents.shape) != (B, S_img, c_lat):
            raise ValueError(f"latents must be packed [B, S, {c_lat}] = {(B, S_img, c_lat)}, got {tuple(latents.shape)}")
        # generator order: only the noise; the reference latents are the posterior's mode
        lat, _, _ = self.prepare_latents(B, height, width, generator, latents)
        reference = None
        if ref_hw:
            made = [(mk(), reference_ids(hr // 2, wr // 2, lat.device)) for (hr, wr), mk in zip(ref_hw, ref_make)]
            reference = [made[b % len(made)] for b in range(B)]
        sig = self.scheduler.sigmas(num_inference_steps, S_img)
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_eff = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float()) \
            if tr.config.guidance_embeds else 0.0
        xs = self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff,
                                  reference=reference, cfg=cfg)
        return self._finish(xs, h, w, output_type, return_dict)
