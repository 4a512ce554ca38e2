"""`FluxFillPipelineRewritePrompt`: FLUX.1 Fill (context-aware inpainting / outpainting) on the MI355X HIP engine.

[ext] diffusers >= 0.32 `FluxFillPipeline.__call__` (image=, mask_image=) on top of `FluxImg2ImgPipelineRewritePrompt`, so
`prompt_embeds` of any length -- the ThinkDiff aligner's tokens -- drive a fill that reads what surrounds the hole.  **Parity
unpinned**: diffusers is not installed (and the rest of the repository follows 0.31.0, which has no Fill pipeline); the semantics
are restated from its published sources (`pipeline_flux_fill.py`, `image_processor.py`) and THIS TEXT IS THE CONTRACT the tests
check.  B = prompts x num_images_per_prompt, h = H/8, w = W/8, C = 16, S = (H/16)(W/16); H and W are multiples of 16.

- The transformer is the channel-conditioned one: `in_channels == 64 + 64 + 256 == 384`, `out_channels == 64`.  Per image a
  condition [S, 320] is concatenated to the latents [S, 64] along the channel axis in front of EVERY transformer call; `x_embedder`
  reads the 384 columns in one Linear, `proj_out` writes 64.  Here the condition is written once per image into the engine
  context that carries the sample (`FluxTransformer2DModel.set_channel_condition`) and the engine gathers the latents beside it.
- Schedule: the FULL text-to-image schedule `sigmas(N, S)` from pure noise; there is no `strength`.
- Generator order: the noise first, `randn([B, 16, h, w], generator, device, bf16)` (skipped when packed `latents` [B, S, 64] are
  given, as in the text-to-image pipeline), THEN eps `[B_img, 16, h, w]` of the masked image's posterior sample (skipped with
  `masked_image_latents`).
- Mask: `preprocess_mask` of flux_inpaint.py unchanged (PIL masks resized with LANCZOS in their own mode, then "L"; float tensor
  masks must already be height x width), binarized on the GPU (u8 >= 128, float >= 0.5).  `check_batches` as there; sample b takes
  prompt b // num_images_per_prompt, image b % B_img and mask b % B_m.
- Masked image: `masked_image = preprocess(image) * (1 - mask)` in fp32, `.to(bf16)`, at FULL pixel resolution: fused into the
  encoder's image-in kernel (td_vae_encode_masked).
- Condition of (image i, mask m) -- td_flux_fill_condition, one pass:
      columns 0..63:    _pack_latents((latent_dist.sample(eps[i]) - shift_factor) * scaling_factor)      (bf16 ops, as img2img's)
      columns 64..319:  the binarized mask UNSHUFFLED, not sampled: mask[H, W].view(h, 8, w, 8).permute(1, 3, 0, 2) -> [64, h, w]
                        -> _pack_latents: column 64 + (py*8 + px)*4 + dy*2 + dx of token (Y, X) = m[8(2Y+dy) + py, 8(2X+dx) + px]
  `masked_image_latents` (packed [B, S, 320]) replaces all of this, the eps draw included.
- Loop: the plain Euler loop of the text-to-image pipeline (td_flux_denoise / _multi): no blend, the output is not composited
  with the input.  Output: `_finish` as in the other pipelines.

Refused, not approximated (NotImplementedError): `callback_on_step_end`, custom `sigmas`, lists of generators,
`joint_attention_kwargs` (the per-call LoRA scale: adapters loaded with `load_lora_weights` are merged into the weights, so set their
weights with `set_adapters(names, weights)` before the call).  A transformer with other channel counts is refused with both numbers named.
"""
from typing import Optional

import torch

from .. import _hip
from .flux_img2img import FluxImg2ImgPipelineRewritePrompt
from .flux_inpaint import check_batches, preprocess_mask
from .flux_prompt import latent_channels
from .flux_transformer import _OPS, effective_scalar

MASK_CHANNELS = 256      # an 8 x 8 pixel block per latent pixel, 2 x 2 latent pixels per token


def refuse_unsupported(name: str, generator, kw: dict) -> None:
    """What the channel-conditioned pipelines refuse before anything runs (shared by Fill and Control)."""
    for key in ("callback_on_step_end", "sigmas", "joint_attention_kwargs"):
        if kw.get(key) is not None:
            raise NotImplementedError(f"{key} is not supported by {name}")
    if isinstance(generator, (list, tuple)):
        raise NotImplementedError("a list of generators is not supported: pass one generator")


def require_channels(name: str, config, in_channels: int, out_channels: int) -> None:
    got_in, got_out = int(config.in_channels), latent_channels(config)
    if (got_in, got_out) != (in_channels, out_channels):
        raise ValueError(f"{name} needs a transformer with in_channels == {in_channels} and out_channels == {out_channels}; "
                         f"this one has in_channels = {got_in}, out_channels = {got_out}")


def unshuffle_mask(mask: torch.Tensor) -> torch.Tensor:
    """[ext] FluxFillPipeline.prepare_mask_latents on one binarized mask [H, W]: view(h, 8, w, 8).permute(1, 3, 0, 2) -> [64, h, w] ->
    _pack_latents -> [S, 256].  Eager torch, any device: the statement td_flux_fill_condition's mask columns restate."""
    H, W = mask.shape
    h, w = H // 8, W // 8
    m = mask.view(h, 8, w, 8).permute(1, 3, 0, 2).reshape(64, h, w)
    return m.view(64, h // 2, 2, w // 2, 2).permute(1, 3, 0, 2, 4).reshape((h // 2) * (w // 2), 256)


class FluxFillPipelineRewritePrompt(FluxImg2ImgPipelineRewritePrompt):
    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, image=None, mask_image=None, masked_image_latents=None, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 50, guidance_scale: float = 30.0, num_images_per_prompt: int = 1,
                 generator=None, latents=None, prompt_embeds=None, pooled_prompt_embeds=None, output_type: str = "pil",
                 return_dict: bool = True, max_sequence_length: int = 512, **kw):
        name = type(self).__name__
        refuse_unsupported(name, generator, kw)
        tr = self.transformer
        c_lat = 64
        require_channels(name, tr.config, c_lat + c_lat + MASK_CHANNELS, c_lat)
        height = int(height or self.default_sample_size * self.vae_scale_factor)
        width = int(width or self.default_sample_size * self.vae_scale_factor)
        if height % 16 or width % 16:
            raise ValueError(f"height and width must be multiples of 16, got {height} x {width}")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if masked_image_latents is None and (image is None or mask_image is None):
            raise ValueError("Provide `image` and `mask_image` (or packed `masked_image_latents`).")
        if masked_image_latents is None:
            masks = preprocess_mask(mask_image, height, width)
            imgs = self._image_list(image, height, width)
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        B = prompt_embeds.shape[0] * num_images_per_prompt
        c, h, w = c_lat // 4, height // 8, width // 8
        S_img = (h // 2) * (w // 2)
        if masked_image_latents is None:
            check_batches(B, len(imgs), len(masks))
        elif tuple(masked_image_latents.shape) != (B, S_img, c_lat + MASK_CHANNELS):
            raise ValueError(f"masked_image_latents must be packed [B, S, {c_lat + MASK_CHANNELS}] = {(B, S_img, c_lat + MASK_CHANNELS)}, "
                             f"got {tuple(masked_image_latents.shape)}")
        if latents is not None and tuple(latents.shape) != (B, S_img, c_lat):
            raise ValueError(f"latents must be packed [B, S, {c_lat}] = {(B, S_img, c_lat)}, got {tuple(latents.shape)}")
        if masked_image_latents is None and self.vae_encoder is None:
            raise _hip.ThinkDiffHipError("no VAE encoder loaded: build the pipeline with vae_encoder= (or from_pipe / from_pretrained)")
        dev = self._execution_device
        # generator order: the noise, then the masked image's eps
        lat, _, _ = self.prepare_latents(B, height, width, generator, latents)
        if masked_image_latents is not None:
            conds = [masked_image_latents[b].to(dev, torch.bfloat16).contiguous() for b in range(B)]
        else:
            eps = torch.randn((len(imgs), c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
            enc, made, conds = self.vae_encoder, {}, []
            for b in range(B):
                i, m = b % len(imgs), b % len(masks)
                if (i, m) not in made:
                    mask_d = masks[m].to(dev)
                    mom = enc.encode_moments(imgs[i], mask=mask_d)
                    made[(i, m)] = _OPS.flux_fill_condition(mom, eps[i], mask_d, float(self.vae_scaling_factor), float(self.vae_shift_factor),
                                                            height, width)
                conds.append(made[(i, m)])
        sig = self.scheduler.sigmas(num_inference_steps, S_img)
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_eff = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float()) \
            if tr.config.guidance_embeds else 0.0
        xs = self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff,
                                  channel_cond=conds)
        return self._finish(xs, h, w, output_type, return_dict)
