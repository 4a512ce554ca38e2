"""`FluxControlPipelineRewritePrompt`: FLUX.1 Canny / Depth (structure-guided rendering) on the MI355X HIP engine.

[ext] diffusers >= 0.32 `FluxControlPipeline.__call__` (control_image=) on top of `FluxImg2ImgPipelineRewritePrompt`, so
`prompt_embeds` of any length -- the ThinkDiff aligner's tokens -- drive a render that follows an edge or depth map.  **Parity
unpinned**: diffusers is not installed (and the rest of the repository follows 0.31.0, which has no Control pipeline); the
semantics are restated from its published sources (`pipeline_flux_control.py`) and THIS TEXT IS THE CONTRACT the tests check.
B = prompts x num_images_per_prompt, h = H/8, w = W/8, C = 16, S = (H/16)(W/16); H and W are multiples of 16.

- The transformer is the channel-conditioned one: `in_channels == 128`, `out_channels == 64`: the packed control-image latents
  [S, 64] are concatenated to the latents [S, 64] along the channel axis in front of EVERY transformer call (FLUX.1 Fill's
  construction with a 64-channel condition; flux_fill.py).  Here they are written once per image into the engine context that
  carries the sample (`FluxTransformer2DModel.set_channel_condition`).
- Generator order: eps `[B_img, 16, h, w]` of the control image's posterior sample FIRST, then the noise `[B, 16, h, w]` (skipped
  when packed `latents` [B, S, 64] are given), both `torch.randn(..., generator, device, bf16)`.
- Condition of control image i: `_pack_latents((latent_dist.sample(eps[i]) - shift_factor) * scaling_factor)` -- the encoder and
  td_vae_latents_from_moments without noise, exactly img2img's clean latents.  Control images are preprocessed like img2img's images
  (PIL resized with LANCZOS; float tensors [B, 3, H, W] in [0, 1] must already be height x width).  Sample b takes prompt b //
  num_images_per_prompt and control image b % B_img; B_img must divide B.
- A `control_image` tensor [B_img, 16, h, w] is taken as latents: packed as it is, no encoder pass, no shift / scale, no eps draw.
- Schedule and loop: the full text-to-image schedule from pure noise, the plain Euler loop (td_flux_denoise / _multi); `_finish`
  as in the other pipelines.

Refused, not approximated (NotImplementedError): `callback_on_step_end`, custom `sigmas`, lists of generators,
`joint_attention_kwargs` (the per-call LoRA scale: adapters loaded with `load_lora_weights` are merged into the weights, so set their
weights with `set_adapters(names, weights)`; the FLUX.1 Canny / Depth *LoRA* checkpoints, which widen `x_embedder`, are refused by the
loader -- the full 128-channel ones load).  The
ControlNet side network is a different model with its own pipeline (flux_controlnet.py), not this one.  A transformer with other channel counts is refused with
both numbers named.
"""
from typing import Optional

import torch

from .. import _hip
from .flux_fill import refuse_unsupported, require_channels
from .flux_img2img import FluxImg2ImgPipelineRewritePrompt
from .flux_transformer import _OPS, effective_scalar
from .flux_vae import DiagonalGaussianDistribution


class FluxControlPipelineRewritePrompt(FluxImg2ImgPipelineRewritePrompt):
    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, control_image=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 28, guidance_scale: float = 3.5, num_images_per_prompt: int = 1, generator=None, latents=None,
                 prompt_embeds=None, pooled_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
                 max_sequence_length: int = 512, **kw):
        name = type(self).__name__
        refuse_unsupported(name, generator, kw)
        tr = self.transformer
        c_lat = 64
        require_channels(name, tr.config, 2 * c_lat, c_lat)
        height = int(height or self.default_sample_size * self.vae_scale_factor)
        width = int(width or self.default_sample_size * self.vae_scale_factor)
        if height % 16 or width % 16:
            raise ValueError(f"height and width must be multiples of 16, got {height} x {width}")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if control_image is None:
            raise ValueError("Provide `control_image`.")
        c, h, w = c_lat // 4, height // 8, width // 8
        S_img = (h // 2) * (w // 2)
        as_latents = isinstance(control_image, torch.Tensor) and control_image.dim() == 4 and control_image.shape[1] == c
        if as_latents:
            if tuple(control_image.shape[2:]) != (h, w):
                raise ValueError(f"a {c}-channel control_image is taken as latents and must be [B, {c}, h, w] with (h, w) = {(h, w)}, "
                                 f"got {tuple(control_image.shape)}")
            n_ctrl = control_image.shape[0]
        else:
            imgs = self._image_list(control_image, height, width)
            n_ctrl = len(imgs)
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        B = prompt_embeds.shape[0] * num_images_per_prompt
        if B % n_ctrl:
            raise ValueError(f"cannot duplicate {n_ctrl} control images to the batch of {B} (prompts x num_images_per_prompt)")
        if latents is not None and tuple(latents.shape) != (B, S_img, c_lat):
            raise ValueError(f"latents must be packed [B, S, {c_lat}] = {(B, S_img, c_lat)}, got {tuple(latents.shape)}")
        if not as_latents and self.vae_encoder is None:
            raise _hip.ThinkDiffHipError("no VAE encoder loaded: build the pipeline with vae_encoder= (or from_pipe / from_pretrained)")
        dev = self._execution_device
        # generator order: the control image's eps, then the noise
        if as_latents:
            ctrl = [_OPS.flux_pack_latents(control_image[i].to(dev, torch.bfloat16).contiguous()) for i in range(n_ctrl)]
        else:
            enc = self.vae_encoder
            moments = [enc.encode_moments(im) for im in imgs]
            eps = torch.randn((n_ctrl, c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
            dist = DiagonalGaussianDistribution(moments, h, w)
            ctrl = [dist.packed_latents(i, eps[i], None, 0.0, self.vae_scaling_factor, self.vae_shift_factor) for i in range(n_ctrl)]
        lat, _, _ = self.prepare_latents(B, height, width, generator, latents)
        conds = [ctrl[b % n_ctrl] for b in range(B)]
        sig = self.scheduler.sigmas(num_inference_steps, S_img)
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_eff = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float()) \
            if tr.config.guidance_embeds else 0.0
        xs = self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff,
                                  channel_cond=conds)
        return self._finish(xs, h, w, output_type, return_dict)
