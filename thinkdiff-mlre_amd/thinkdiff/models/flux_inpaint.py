"""`FluxInpaintPipelineRewritePrompt`: FLUX inpainting on the MI355X HIP engine.

[ext] diffusers 0.31.0 `FluxInpaintPipeline.__call__` (image=, mask_image=, strength=) on top of
`FluxImg2ImgPipelineRewritePrompt`, so `prompt_embeds` of any length -- the ThinkDiff aligner's tokens -- drive a local edit as
they drive img2img.  Parity unpinned: diffusers is not installed; the semantics are restated from its published sources
(`pipeline_flux_inpaint.py`, `image_processor.py`, `scheduling_flow_match_euler_discrete.py`).  B = prompts x
num_images_per_prompt, latents h = H/8, w = W/8, C = 16, S = (H/16)(W/16); H and W are multiples of 16 (the encoder's rule).

- Schedule: as img2img, t_start = `get_timesteps(N, strength)`; the loop runs sig = sigmas(N, S)[t_start:].
- `mask_processor` (grayscale, no normalisation, binarize): PIL masks are resized on the host to (width, height) with LANCZOS in
  their own mode, only when the size differs (PIL itself uses NEAREST for modes "1" and "P"), then `convert("L")` -- the order of
  `VaeImageProcessor.preprocess`.  Float tensors [H, W], [1, H, W] or [B_m, 1, H, W] in [0, 1] must already be height x width (no
  tensor resizing).  On the GPU, one kernel (td_flux_inpaint_mask) binarizes in fp32 (u8 / 255 >= 0.5, i.e. u8 >= 128; v >= 0.5),
  takes mask pixel (8y, 8x) for latent pixel (y, x) (`F.interpolate(nearest)` at the exact factor 8), repeats it over the 16
  channels and packs it: bf16 [S, 64] of 0 / 1.
- `prepare_latents` / `prepare_mask_latents`, in generator order: eps [B_img, 16, h, w] of the image's posterior sample, then the
  noise [B, 16, h, w] (only when `latents` is None), then one more bf16 draw [max(B_img, B_m), 16, h, w] that stands for the masked
  image's posterior sample.  The 64-channel transformer never reads the masked-image latents, so the encoder does not run for them;
  the draw is made and dropped so that a reused generator continues as diffusers leaves it (skipped when `masked_image_latents` with
  16 channels is passed).  Every draw is `torch.randn(..., generator, device, bf16)`.  Sample b takes prompt b //
  num_images_per_prompt, image b % B_img and mask b % B_m; B_img and B_m must divide B, and be equal or one of them 1.
- Clean latents z_b = pack((sample(image) - shift) * scaling) and the start point x_b = scale_noise(z_b, bf16(sig[0]), noise_b) are
  td_vae_latents_from_moments without / with the noise.  `latents=` are UNPACKED bf16 [B, 16, h, w] here (unlike img2img's packed
  ones): they are the start point, not re-noised, and the blend's noise; the image is still encoded, because the blend needs z.
- Loop step i of n = len(sig) - 1 (td_flux_denoise_inpaint; flux_inpaint_step_ is the step alone), torch's bf16 rounding points:
      a  = bf16(float(x) + float(bf16(bf16(dt) * float(v))))          dt = sig[i+1] - sig[i]
      s  = bf16(sig[i+1])
      p  = i < n-1 ? bf16(bf16(s * noise) + bf16(bf16(1 - s) * z)) : z
      x' = bf16(bf16(bf16(1 - m) * p) + bf16(m * a))
- Output: `_finish` as in the other pipelines; no overlay (that needs `padding_mask_crop`).

Refused, not approximated: `padding_mask_crop` (crop region, resize_mode="fill", apply_overlay), resizing tensor masks,
`callback_on_step_end`, custom `sigmas` and lists of generators.  FLUX.1 Fill (the 384-channel transformer that reads the
masked-image latents) is a pipeline of its own: `FluxFillPipelineRewritePrompt` (flux_fill.py).
"""
from typing import List, Optional

import numpy as np
import torch

from .. import _hip
from .flux_img2img import FluxImg2ImgPipelineRewritePrompt, get_timesteps
from .flux_transformer import _OPS, effective_scalar
from .flux_vae import DiagonalGaussianDistribution


def preprocess_mask(mask_image, height: int, width: int) -> List[torch.Tensor]:
    """[ext] `mask_processor.preprocess` up to the binarization (host side): PIL masks -> uint8 [H, W] CPU tensors (resize with LANCZOS
    in the image's own mode when the size differs, then convert("L")); float tensors -> float32 [H, W] tensors, one per mask."""
    from PIL import Image
    if isinstance(mask_image, Image.Image):
        mask_image = [mask_image]
    if isinstance(mask_image, torch.Tensor):
        m = mask_image
        if not m.is_floating_point():
            raise ValueError(f"mask tensors must be float in [0, 1], got {m.dtype}")
        if m.dim() == 2:
            m = m[None, None]
        elif m.dim() == 3 and m.shape[0] == 1:
            m = m[None]
        if m.dim() != 4 or m.shape[1] != 1:
            raise ValueError(f"mask tensors must be [H, W], [1, H, W] or [B, 1, H, W], got {tuple(mask_image.shape)}")
        if tuple(m.shape[2:]) != (height, width):
            raise ValueError(f"mask tensor is {tuple(m.shape[2:])}, expected (height, width) = {(height, width)}: "
                             "tensor masks are not resized (resize on the host, or pass PIL masks)")
        return [m[i, 0].float().contiguous() for i in range(m.shape[0])]
    out = []
    for im in mask_image:
        if not isinstance(im, Image.Image):
            raise ValueError(f"mask_image must be a PIL image, a list of them or a float tensor, got {type(im)}")
        if im.size != (width, height):
            im = im.resize((width, height), resample=Image.LANCZOS)
        out.append(torch.from_numpy(np.array(im.convert("L"), dtype=np.uint8)))
    return out


def check_batches(B: int, n_images: int, n_masks: int) -> None:
    """[ext] prepare_latents / prepare_mask_latents repeat the image and mask batches to B, and `init_image * (mask < 0.5)` must broadcast."""
    if B % n_images:
        raise ValueError(f"cannot duplicate {n_images} images to the batch of {B} (prompts x num_images_per_prompt)")
    if B % n_masks:
        raise ValueError(f"cannot duplicate {n_masks} masks to the batch of {B} (prompts x num_images_per_prompt)")
    if n_images != n_masks and 1 not in (n_images, n_masks):
        raise ValueError(f"{n_images} images and {n_masks} masks: pass as many masks as images, or one of either")


class FluxInpaintPipelineRewritePrompt(FluxImg2ImgPipelineRewritePrompt):
    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, image=None, mask_image=None, masked_image_latents=None, height: Optional[int] = None,
                 width: Optional[int] = None, padding_mask_crop: Optional[int] = None, strength: float = 0.6, num_inference_steps: int = 28,
                 guidance_scale: float = 7.0, num_images_per_prompt: int = 1, generator=None, latents=None, prompt_embeds=None,
                 pooled_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True, max_sequence_length: int = 512, **kw):
        self._refuse_call_scale(kw)      # (a per-call LoRA scale while adapters are loaded: set_adapters(names, weights) instead)
        if padding_mask_crop is not None:
            raise NotImplementedError("padding_mask_crop (crop region, resize_mode='fill', apply_overlay) is not supported")
        for name in ("callback_on_step_end", "sigmas"):
            if kw.get(name) is not None:
                raise NotImplementedError(f"{name} is not supported by FluxInpaintPipelineRewritePrompt")
        if isinstance(generator, (list, tuple)):
            raise NotImplementedError("a list of generators is not supported: pass one generator")
        height = int(height or self.default_sample_size * self.vae_scale_factor)
        width = int(width or self.default_sample_size * self.vae_scale_factor)
        if height % 16 or width % 16:
            raise ValueError(f"height and width must be multiples of 16, got {height} x {width}")
        t_start = get_timesteps(num_inference_steps, strength)
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if image is None or mask_image is None:
            raise ValueError("Provide `image` and `mask_image`.")
        masks = preprocess_mask(mask_image, height, width)
        imgs = self._image_list(image, height, width)
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        tr = self.transformer
        B = prompt_embeds.shape[0] * num_images_per_prompt
        check_batches(B, len(imgs), len(masks))
        c = tr.config.in_channels // 4
        h, w = height // 8, width // 8
        if latents is not None and tuple(latents.shape) != (B, c, h, w):
            raise ValueError(f"latents must be unpacked [B, {c}, h, w] = {(B, c, h, w)} for the inpainting pipeline, got {tuple(latents.shape)}")
        if self.vae_encoder is None:
            raise _hip.ThinkDiffHipError("no VAE encoder loaded: build the pipeline with vae_encoder= (or from_pipe / from_pretrained)")
        S_img = (h // 2) * (w // 2)
        sig = self.scheduler.sigmas(num_inference_steps, S_img)[t_start:]
        dev = self._execution_device
        enc = self.vae_encoder
        moments = [enc.encode_moments(im) for im in imgs]
        eps = torch.randn((len(imgs), c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
        noise = None if latents is not None else torch.randn((B, c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
        if masked_image_latents is None or masked_image_latents.shape[1] != c:
            n_masked = max(len(imgs), len(masks)) if masked_image_latents is None else masked_image_latents.shape[0]
            torch.randn((n_masked, c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)    # the masked image's sample, dropped
        dist = DiagonalGaussianDistribution(moments, h, w)
        z = [dist.packed_latents(i, eps[i], None, 0.0, self.vae_scaling_factor, self.vae_shift_factor) for i in range(len(imgs))]
        mask_lat = [_OPS.flux_inpaint_mask(m.to(dev), c) for m in masks]
        blend, start = [], []
        for b in range(B):
            i = b % len(imgs)
            if latents is None:
                nb = _OPS.flux_pack_latents(noise[b])
                start.append(dist.packed_latents(i, eps[i], noise[b], float(sig[0]), self.vae_scaling_factor, self.vae_shift_factor))
            else:              # diffusers: the given latents are the start point and the noise (the engine writes the start point: a copy)
                nb = _OPS.flux_pack_latents(latents[b].to(dev, torch.bfloat16).contiguous())
                start.append(nb.clone())
            blend.append((z[i], nb, mask_lat[b % len(masks)]))
        lat = torch.stack(start)
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_eff = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float()) \
            if tr.config.guidance_embeds else 0.0
        xs = self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff,
                                  inpaint=blend)
        return self._finish(xs, h, w, output_type, return_dict)
