"""`FluxImg2ImgPipelineRewritePrompt`: FLUX image-to-image on the MI355X HIP engine.

[ext] diffusers 0.31.0 `FluxImg2ImgPipeline.__call__` (image=, strength=) on top of `FluxPipelineRewritePrompt`, so
`prompt_embeds` of any length -- the ThinkDiff aligner's tokens -- drive it as they drive text-to-image.  Parity unpinned:
diffusers is not installed; the semantics are restated from its published sources:

- `VaeImageProcessor.preprocess`: PIL images are resized on the host with LANCZOS to height x width; the 2x - 1 normalisation
  and the bf16 cast run on the GPU in front of the encoder.  Float tensors [B, 3, H, W] in [0, 1] must already be height x width
  (a documented simplification: no tensor resizing).
- `get_timesteps`: init = min(N * strength, N), t_start = int(max(N - init, 0)); the loop runs `sigmas[t_start:]` of the
  text-to-image schedule, N - t_start transformer forwards.
- `prepare_latents`: eps of the posterior sample is drawn first ([B_img, 16, h, w]), then the noise ([B, 16, h, w]), both
  `torch.randn(..., generator, device, bf16)`; sample b starts from image b % B_img (diffusers repeats the encoded batch);
  `latents=` skips the encoder.
- `_encode_vae_image` shift / scale, `scale_noise` at sigma = bf16(sigmas[t_start]) and `_pack_latents` are one fused kernel
  (td_vae_latents_from_moments).
"""
from typing import Optional

import numpy as np
import torch

from .. import _hip
from .flux_prompt import FluxPipelineRewritePrompt
from .flux_transformer import effective_scalar
from .flux_vae import AutoencoderKL, AutoencoderKLDecoder, AutoencoderKLEncoder, DiagonalGaussianDistribution


def get_timesteps(num_inference_steps: int, strength: float) -> int:
    """[ext] FluxImg2ImgPipeline.get_timesteps: the index of the first sigma the loop runs (it runs N - t_start steps)."""
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"The value of strength should be in [0.0, 1.0] but is {strength}")
    init_timestep = min(num_inference_steps * strength, num_inference_steps)
    t_start = int(max(num_inference_steps - init_timestep, 0))
    if num_inference_steps - t_start < 1:
        raise ValueError(f"strength {strength} with num_inference_steps {num_inference_steps} leaves no denoising step")
    return t_start


class FluxImg2ImgPipelineRewritePrompt(FluxPipelineRewritePrompt):
    def __init__(self, *args, vae_encoder: Optional[AutoencoderKLEncoder] = None, **kw):
        super().__init__(*args, **kw)
        if vae_encoder is not None:
            if not isinstance(self.vae, AutoencoderKLDecoder):
                raise _hip.ThinkDiffHipError("vae_encoder needs the pipeline's VAE decoder (vae=AutoencoderKLDecoder)")
            self.vae = AutoencoderKL(vae_encoder, self.vae)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=torch.bfloat16, max_image_size=(1024, 1024), **kw):
        """Transformer, full VAE (encoder and decoder: vae/ is required) and text encoders, from a local diffusers-layout directory."""
        pipe = super().from_pretrained(pretrained_model_name_or_path, torch_dtype, **kw)
        if pipe.vae is None:
            raise FileNotFoundError(f"{pretrained_model_name_or_path!r} has no vae/ folder: image-to-image needs the VAE encoder")
        pipe.vae = AutoencoderKL(AutoencoderKLEncoder.from_pretrained(pretrained_model_name_or_path, max_image_size=max_image_size), pipe.vae)
        return pipe

    @classmethod
    def from_pipe(cls, pipe: FluxPipelineRewritePrompt, vae_encoder: AutoencoderKLEncoder):
        """Shares the transformer, its forked contexts and streams, the VAE decoder and the text encoders of `pipe`."""
        new = cls(scheduler=pipe.scheduler, vae=pipe.vae, text_encoder=pipe.text_encoder, tokenizer=pipe.tokenizer,
                  text_encoder_2=pipe.text_encoder_2, tokenizer_2=pipe.tokenizer_2, transformer=pipe.transformer, vae_encoder=vae_encoder)
        new._ctx_pool, new._streams = pipe._ctx_pool, pipe._streams
        new.images_in_flight = pipe.images_in_flight
        new.vae_scale_factor = pipe.vae_scale_factor
        return new

    @property
    def vae_encoder(self) -> Optional[AutoencoderKLEncoder]:
        return getattr(self.vae, "encoder", None)

    def _image_list(self, image, height: int, width: int):
        """[ext] VaeImageProcessor.preprocess up to the normalisation: device tensors, uint8 [H, W, 3] (PIL) or float [3, H, W]."""
        from PIL import Image
        if isinstance(image, Image.Image):
            image = [image]
        if isinstance(image, torch.Tensor):
            if image.dim() == 3:
                image = image[None]
            if image.dim() != 4 or image.shape[1] != 3 or not image.is_floating_point():
                raise ValueError(f"image tensors must be float [B, 3, H, W] in [0, 1], got {tuple(image.shape)} {image.dtype}")
            if tuple(image.shape[2:]) != (height, width):
                raise ValueError(f"image tensor is {tuple(image.shape[2:])}, expected (height, width) = {(height, width)}: "
                                 "tensor inputs are not resized (resize on the host, or pass PIL images)")
            return [image[i].float().contiguous() for i in range(image.shape[0])]
        out = []
        for im in image:
            if not isinstance(im, Image.Image):
                raise ValueError(f"image must be a PIL image, a list of them or a float tensor, got {type(im)}")
            im = im.convert("RGB")
            if im.size != (width, height):
                im = im.resize((width, height), resample=Image.LANCZOS)
            out.append(torch.from_numpy(np.array(im, dtype=np.uint8)))
        return out

    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, image=None, strength: float = 0.6, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 28, guidance_scale: float = 7.0,
                 num_images_per_prompt: int = 1, generator=None, latents=None, prompt_embeds=None, pooled_prompt_embeds=None,
                 output_type: str = "pil", return_dict: bool = True, max_sequence_length: int = 512, **_ignored):
        self._refuse_call_scale(_ignored)      # (a per-call LoRA scale while adapters are loaded: set_adapters(names, weights) instead)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        t_start = get_timesteps(num_inference_steps, strength)
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if image is None and latents is None:
            raise ValueError("Provide `image` (or packed `latents`).")
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        tr = self.transformer
        B = prompt_embeds.shape[0] * num_images_per_prompt
        c = tr.config.in_channels // 4
        h = 2 * (int(height) // self.vae_scale_factor)
        w = 2 * (int(width) // self.vae_scale_factor)
        S_img = (h // 2) * (w // 2)
        sig = self.scheduler.sigmas(num_inference_steps, S_img)[t_start:]
        if latents is not None:          # diffusers: given latents are the start point, the image is not encoded
            lat, h, w = self.prepare_latents(B, height, width, generator, latents)
        else:
            if self.vae_encoder is None:
                raise _hip.ThinkDiffHipError("no VAE encoder loaded: build the pipeline with vae_encoder= (or from_pipe / from_pretrained)")
            imgs = self._image_list(image, int(height), int(width))
            if len(imgs) not in (1, prompt_embeds.shape[0]):
                raise ValueError(f"{len(imgs)} images for {prompt_embeds.shape[0]} prompts: pass one image or one per prompt")
            enc = self.vae_encoder
            moments = [enc.encode_moments(im) for im in imgs]
            dev = self._execution_device
            eps = torch.randn((len(imgs), c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
            noise = torch.randn((B, c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
            dist = DiagonalGaussianDistribution(moments, h, w)
            lat = torch.stack([dist.packed_latents(b % len(imgs), eps[b % len(imgs)], noise[b], float(sig[0]),
                                                   self.vae_scaling_factor, self.vae_shift_factor) for b in range(B)])
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_eff = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float()) \
            if tr.config.guidance_embeds else 0.0
        xs = self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff)
        return self._finish(xs, h, w, output_type, return_dict)
