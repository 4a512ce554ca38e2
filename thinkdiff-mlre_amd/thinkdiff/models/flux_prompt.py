"""`FluxPipelineRewritePrompt` on the MI355X HIP engine.

Drop-in for reference `thinkdiff/models/flux_prompt.py:16-121` (a `diffusers.FluxPipeline` subclass
whose `encode_prompt` lets callers inject `prompt_embeds` of any length) together with the inherited
[ext] diffusers 0.31.0 `FluxPipeline.__call__` the drivers invoke
(scripts/test/test_blip_vision_t5_decoder_flux_text.py:234-242).  Same names, argument meaning and
return shapes; the denoise loop itself runs in libthinkdiff_hip.so (`td_flux_*`).

What is host-side here is only scalar schedule arithmetic and argument plumbing.  Text encoders
(CLIP-L / T5-XXL) and the VAE are optional components (SURVEY.md 8f "next" rows): without a VAE the
call returns latents (`output_type="latent"`).
"""
import math
from types import SimpleNamespace
from typing import List, Optional, Union

import numpy as np
import torch

from .. import _hip
from ..ops import register as _register_ops
from .flux_transformer import FluxTransformer2DModel, FluxTransformerConfig, effective_scalar
_OPS = _register_ops()      # torch.ops.thinkdiff_hip: the custom-op layer over the C ABI (GPU kernels only, no fallback)


class FlowMatchEulerSchedule:
    """Scalar part of [ext] FlowMatchEulerDiscreteScheduler with the FLUX.1-dev scheduler_config.json
    (use_dynamic_shifting, base_shift 0.5, max_shift 1.15, base/max_image_seq_len 256/4096)."""
    base_image_seq_len, max_image_seq_len, base_shift, max_shift = 256, 4096, 0.5, 1.15
    num_train_timesteps = 1000

    @classmethod
    def calculate_shift(cls, image_seq_len: int) -> float:
        m = (cls.max_shift - cls.base_shift) / (cls.max_image_seq_len - cls.base_image_seq_len)
        return image_seq_len * m + (cls.base_shift - m * cls.base_image_seq_len)

    @classmethod
    def sigmas(cls, num_inference_steps: int, image_seq_len: int) -> np.ndarray:
        s = np.linspace(1.0, 1.0 / num_inference_steps, num_inference_steps)
        mu = cls.calculate_shift(image_seq_len)
        s = math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0) ** 1.0)
        return np.concatenate([s.astype(np.float32), np.zeros(1, dtype=np.float32)])


def latent_channels(config) -> int:
    """Width of the packed latents of a transformer config: `out_channels` where the config has one (channel-conditioned checkpoints read
    more than they write), else `in_channels`."""
    return int(getattr(config, "out_channels", None) or config.in_channels)


class FluxPipelineRewritePrompt:
    vae_scale_factor = 16          # [ext] FluxPipeline.__init__ (0.31.0): 2 ** len(vae.block_out_channels)
    vae_scaling_factor = 0.3611    # [ext] FLUX.1-dev vae/config.json
    vae_shift_factor = 0.1159
    default_sample_size = 64

    def __init__(self, scheduler=None, vae=None, text_encoder=None, tokenizer=None, text_encoder_2=None,
                 tokenizer_2=None, transformer: Optional[FluxTransformer2DModel] = None):
        self.scheduler = scheduler or FlowMatchEulerSchedule()
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2
        self.transformer = transformer
        self._progress = {}
        self.images_in_flight = 2          # images of one call advanced concurrently (engine contexts on separate streams; 2 beats 3 and 4 on MI355X)
        self._ctx_pool, self._streams = [], []

    def _contexts(self, n: int):
        """The transformer plus n-1 forked contexts (created once, shared weights) and one stream per context."""
        if not self._ctx_pool or self._ctx_pool[0] is not self.transformer:
            self._ctx_pool, self._streams = [self.transformer], []
        while len(self._ctx_pool) < n:
            self._ctx_pool.append(self.transformer.fork())
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(device=self.transformer.device))
        return self._ctx_pool[:n]

    # ---- construction --------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=torch.bfloat16, **kw):
        """Local directory in diffusers layout (transformer/ required).  Hub ids cannot be fetched here."""
        import os
        if not os.path.isdir(pretrained_model_name_or_path):
            raise FileNotFoundError(
                f"{pretrained_model_name_or_path!r} is not a local directory; this build loads FLUX weights from "
                "disk only (or use FluxPipelineRewritePrompt.from_random for synthetic weights)")
        from .flux_vae import AutoencoderKLDecoder
        vae = None
        if os.path.isdir(os.path.join(pretrained_model_name_or_path, "vae")):
            vae = AutoencoderKLDecoder.from_pretrained(pretrained_model_name_or_path)
        enc = {}
        root = pretrained_model_name_or_path
        if os.path.isdir(os.path.join(root, "text_encoder")) and os.path.isdir(os.path.join(root, "tokenizer")):
            from transformers import CLIPTokenizer
            from .text_encoders import HipCLIPTextEncoder
            enc.update(text_encoder=HipCLIPTextEncoder.from_pretrained(root), tokenizer=CLIPTokenizer.from_pretrained(os.path.join(root, "tokenizer")))
        if os.path.isdir(os.path.join(root, "text_encoder_2")) and os.path.isdir(os.path.join(root, "tokenizer_2")):
            from transformers import AutoTokenizer
            from .text_encoders import HipT5Encoder
            enc.update(text_encoder_2=HipT5Encoder.from_pretrained(root), tokenizer_2=AutoTokenizer.from_pretrained(os.path.join(root, "tokenizer_2")))
        return cls(transformer=FluxTransformer2DModel.from_pretrained(pretrained_model_name_or_path, **kw), vae=vae, **enc)

    @classmethod
    def from_random(cls, config: Optional[FluxTransformerConfig] = None, seed: int = 0, with_vae: bool = True, **kw):
        """Synthetic FLUX.1-dev-shaped checkpoint created on the device (benchmarks, plumbing tests)."""
        from .flux_vae import AutoencoderKLDecoder
        vae = AutoencoderKLDecoder().init_random(seed + 1) if with_vae else None
        return cls(transformer=FluxTransformer2DModel(config, **kw).init_random(seed), vae=vae)

    # ---- LoRA ([ext] diffusers FluxLoraLoaderMixin) ------------------------------------------------------
    # On this engine adapters are ALWAYS merged into the transformer's weights, recomputed from an untouched base copy whenever the set or
    # its weights change (FluxTransformer2DModel.load_lora_adapter / set_adapters; include/thinkdiff_hip.h td_flux_lora_*): the denoise loop
    # is the same code at the same rate, in every precision, and forked contexts need nothing (they share the weights).  The per-call
    # `joint_attention_kwargs={"scale": s}` is not built: use set_adapters(names, weights).
    def load_lora_weights(self, path_or_dict, weight_name: Optional[str] = None, adapter_name: Optional[str] = None, alpha=None, **_ignored):
        """A local .safetensors file, a directory (+ weight_name, default pytorch_lora_weights.safetensors) or a state dict in the diffusers /
        peft format (thinkdiff.models.flux_lora); no hub.  Transformer adapters only.  The adapter becomes active at weight 1.0 beside those
        already active; alpha= overrides the file's alphas (a number or a dict per module)."""
        if adapter_name is None:
            have, i = set(self.transformer.list_adapters()), 0
            while f"default_{i}" in have:
                i += 1
            adapter_name = f"default_{i}"
        self._fuse_scale = None      # a new active set: fuse_lora's factor belongs to the old one
        self.transformer.load_lora_adapter(path_or_dict, adapter_name=adapter_name, alpha=alpha, weight_name=weight_name)
        return adapter_name

    def set_adapters(self, adapter_names, adapter_weights=None):
        self._fuse_scale = None
        self.transformer.set_adapters(adapter_names, adapter_weights)

    def get_active_adapters(self) -> List[str]:
        return list(self.transformer.active_adapters())

    def get_list_adapters(self):
        return {"transformer": self.transformer.list_adapters()}

    def delete_adapters(self, adapter_names):
        self.transformer.delete_adapters(adapter_names)

    def unload_lora_weights(self):
        self._fuse_scale = None
        self.transformer.unload_lora()

    def fuse_lora(self, lora_scale: float = 1.0, **_ignored):
        """Adapters are merged at all times here; fuse_lora(s) multiplies the active adapters' weights by s until unfuse_lora()."""
        if getattr(self, "_fuse_scale", None) is not None:
            raise ValueError("fuse_lora: already fused (unfuse_lora first)")
        active = self.transformer.active_adapters()
        self._fuse_scale = (float(lora_scale), dict(active))
        if active and float(lora_scale) != 1.0:
            self.transformer.set_adapters(list(active), [w * float(lora_scale) for w in active.values()])

    def unfuse_lora(self, **_ignored):
        """Restores the weights the active adapters had before fuse_lora (the merge is recomputed from the base copy: nothing drifts)."""
        fused, self._fuse_scale = getattr(self, "_fuse_scale", None), None
        if fused is not None and fused[1] and fused[0] != 1.0:
            self.transformer.set_adapters(list(fused[1]), list(fused[1].values()))

    def _refuse_call_scale(self, kwargs):
        """The text-to-image / img2img / inpaint calls swallow unknown keywords; with adapters loaded a per-call LoRA scale must not vanish."""
        jak = kwargs.get("joint_attention_kwargs")
        if jak and "scale" in jak and self.transformer is not None and self.transformer.list_adapters():
            raise NotImplementedError("joint_attention_kwargs={'scale': ...} (a per-call LoRA scale) is not built: adapters are merged into the "
                                      "weights; use set_adapters(names, weights) before the call")

    # ---- IP-Adapter ([ext] diffusers FluxIPAdapterMixin; thinkdiff.models.flux_ip_adapter holds the specification) ----------------------
    def load_ip_adapter(self, path_or_dict, weight_name: Optional[str] = None, image_encoder=None, feature_extractor=None, **_ignored):
        """One adapter from a local .safetensors file, a directory + weight_name, or a state dict (diffusers or XLabs keys); no hub.  Call again
        for a further adapter (up to 4).  image_encoder: an optional torch module whose output has `.image_embeds` (with feature_extractor, if the
        images are not tensors yet) -- it serves `ip_adapter_image`; there is no HIP image encoder, `ip_adapter_image_embeds` needs none."""
        idx = self.transformer.load_ip_adapter(path_or_dict, weight_name=weight_name)
        if image_encoder is not None:
            self.image_encoder, self.feature_extractor = image_encoder, feature_extractor
        return idx

    def set_ip_adapter_scale(self, scale):
        self.transformer.set_ip_adapter_scale(scale)

    def unload_ip_adapter(self):
        for ctx in self._ctx_pool[1:]:
            ctx.set_ip_image_embeds(None)
        self.transformer.unload_ip_adapter()
        self.image_encoder = self.feature_extractor = None

    def encode_image(self, image):
        """`ip_adapter_image` of one adapter (an image, a tensor [n_img, 3, h, w] or a list of images) -> embeds [n_img, E] through the
        caller-supplied image encoder; once per call."""
        enc = getattr(self, "image_encoder", None)
        if enc is None:
            raise ValueError("ip_adapter_image needs an image encoder (load_ip_adapter(..., image_encoder=...)); without one pass ip_adapter_image_embeds")
        if not isinstance(image, torch.Tensor):
            fe = getattr(self, "feature_extractor", None)
            if fe is None:
                raise ValueError("ip_adapter_image: images that are not tensors need a feature_extractor (load_ip_adapter(..., feature_extractor=...))")
            image = fe(images=image, return_tensors="pt").pixel_values
        if image.dim() == 3:
            image = image[None]
        p = next(iter(enc.parameters()), None) if hasattr(enc, "parameters") else None
        if p is not None:
            image = image.to(device=p.device, dtype=p.dtype)
        return enc(image).image_embeds

    def _ip_call_embeds(self, batch, ip_adapter_image, ip_adapter_image_embeds, negative_ip_adapter_image, negative_ip_adapter_image_embeds):
        """The IP arguments of a call -> None, or per adapter a [1 or batch, n_img, E] tensor."""
        from . import flux_ip_adapter as ipa
        if negative_ip_adapter_image is not None or negative_ip_adapter_image_embeds is not None:
            raise NotImplementedError("negative_ip_adapter_image / negative_ip_adapter_image_embeds: a negative image prompt needs true classifier-free "
                                      "guidance, which only FluxKontextPipeline runs here")
        if ip_adapter_image is None and ip_adapter_image_embeds is None:
            return None
        loaded = self.transformer.ip_adapters()
        if not loaded:
            raise ValueError("ip_adapter_image / ip_adapter_image_embeds were passed and no IP-Adapter is loaded (load_ip_adapter first)")
        if ip_adapter_image_embeds is None:
            images = ip_adapter_image if isinstance(ip_adapter_image, list) and len(loaded) > 1 else [ip_adapter_image]
            if len(images) != len(loaded):
                raise ValueError(f"ip_adapter_image: {len(images)} entries for {len(loaded)} loaded adapters (one entry per adapter)")
            ip_adapter_image_embeds = [self.encode_image(im) for im in images]
        return ipa.normalize_image_embeds(ip_adapter_image_embeds, len(loaded), batch, [a["embed_dim"] for a in loaded])

    def to(self, *_a, **_k):
        return self  # the engine lives on the GPU it was created on

    def enable_model_cpu_offload(self, *_a, **_k):
        return None  # 288 GB of HBM: everything stays resident

    def set_progress_bar_config(self, **kw):
        self._progress.update(kw)

    @property
    def _execution_device(self):
        return self.transformer.device

    # ---- reference flux_prompt.py:37-121 ------------------------------------------------------------------
    def encode_prompt(self, prompt: Union[str, List[str], None], prompt_2: Union[str, List[str], None] = None,
                      device=None, num_images_per_prompt: int = 1, prompt_embeds=None, pooled_prompt_embeds=None,
                      max_sequence_length: int = 512, lora_scale=None):
        """Pooled (CLIP) and sequence (T5) embeddings are computed independently, each only when the
        caller did not supply it; text_ids = zeros[T, 3] (no batch dim), T following the embeds."""
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        if pooled_prompt_embeds is None:
            pooled_prompt_embeds = self._get_clip_prompt_embeds(prompt, device, num_images_per_prompt)
        if prompt_embeds is None:
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            prompt_embeds = self._get_t5_prompt_embeds(prompt_2, num_images_per_prompt, max_sequence_length, device)
        dtype = self.transformer.dtype
        text_ids = torch.zeros(prompt_embeds.shape[1], 3).to(device=device, dtype=dtype)
        return prompt_embeds, pooled_prompt_embeds, text_ids

    def _get_clip_prompt_embeds(self, prompt, device, num_images_per_prompt):
        if self.text_encoder is None or self.tokenizer is None:
            raise _hip.ThinkDiffHipError("encode_prompt: no CLIP text encoder loaded; pass pooled_prompt_embeds")
        ids = self.tokenizer(prompt, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        out = self.text_encoder(ids.to(device), output_hidden_states=False).pooler_output
        return out.to(self.transformer.dtype).repeat(1, num_images_per_prompt).view(len(prompt) * num_images_per_prompt, -1)

    def _get_t5_prompt_embeds(self, prompt, num_images_per_prompt, max_sequence_length, device):
        if self.text_encoder_2 is None or self.tokenizer_2 is None:
            raise _hip.ThinkDiffHipError("encode_prompt: no T5 text encoder loaded; pass prompt_embeds")
        ids = self.tokenizer_2(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                               return_tensors="pt").input_ids
        out = self.text_encoder_2(ids.to(device), output_hidden_states=False)[0].to(self.transformer.dtype)
        _, T, _ = out.shape
        return out.repeat(1, num_images_per_prompt, 1).view(len(prompt) * num_images_per_prompt, T, -1)

    # ---- [ext] FluxPipeline helpers -----------------------------------------------------------------------
    @staticmethod
    def _prepare_latent_image_ids(h2: int, w2: int, device) -> torch.Tensor:
        ids = torch.zeros(h2, w2, 3)
        ids[..., 1] += torch.arange(h2)[:, None]
        ids[..., 2] += torch.arange(w2)[None, :]
        return ids.reshape(h2 * w2, 3).to(device)

    def prepare_latents(self, batch: int, height: int, width: int, generator=None, latents=None):
        """Returns packed latents [B, (h/2)(w/2), 64] bf16 and the latent (h, w).  `latents`, if given, is
        already packed (as in diffusers)."""
        c = latent_channels(self.transformer.config) // 4
        h = 2 * (int(height) // self.vae_scale_factor)
        w = 2 * (int(width) // self.vae_scale_factor)
        dev = self._execution_device
        if latents is not None:
            # the engine updates latents in place; diffusers never mutates the caller's tensor, so work on a copy
            return latents.to(dev, torch.bfloat16).contiguous().clone(), h, w
        raw = torch.randn((batch, c, h, w), generator=generator, device=dev, dtype=torch.bfloat16)
        packed = torch.stack([_OPS.flux_pack_latents(raw[b]) for b in range(batch)])
        return packed, h, w

    # ---- the call the drivers make --------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 28, guidance_scale: float = 3.5, num_images_per_prompt: int = 1,
                 generator=None, latents=None, prompt_embeds=None, pooled_prompt_embeds=None,
                 output_type: str = "pil", return_dict: bool = True, max_sequence_length: int = 512, ip_adapter_image=None,
                 ip_adapter_image_embeds=None, negative_ip_adapter_image=None, negative_ip_adapter_image_embeds=None, **_ignored):
        self._refuse_call_scale(_ignored)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        tr = self.transformer
        # [ext] pipeline_flux.py: batch = prompt_embeds.shape[0]; latents for batch * num_images_per_prompt.
        # The reference's encode_prompt does not tile supplied embeds (flux_prompt.py:83-86), so sample b
        # is conditioned on prompt b // num_images_per_prompt.
        B = prompt_embeds.shape[0] * num_images_per_prompt
        # [ext] FluxIPAdapterMixin: the image prompt of sample b is entry b // num_images_per_prompt of every adapter's embeds
        ip_embeds = self._ip_call_embeds(prompt_embeds.shape[0], ip_adapter_image, ip_adapter_image_embeds, negative_ip_adapter_image,
                                         negative_ip_adapter_image_embeds)
        lat, h, w = self.prepare_latents(B, height, width, generator, latents)
        S_img = lat.shape[1]
        img_ids = self._prepare_latent_image_ids(h // 2, w // 2, lat.device)
        sig = self.scheduler.sigmas(num_inference_steps, S_img)
        t_eff = [effective_scalar(float(s) * self.scheduler.num_train_timesteps, tr.dtype) for s in sig[:-1]]
        g_eff = float((torch.tensor([guidance_scale], dtype=torch.float32).to(tr.dtype) * 1000).float()) \
            if tr.config.guidance_embeds else 0.0
        xs = self._denoise_groups(lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff,
                                  ip_embeds=ip_embeds)
        return self._finish(xs, h, w, output_type, return_dict)

    def _denoise_groups(self, lat, B, num_images_per_prompt, prompt_embeds, pooled_prompt_embeds, text_ids, img_ids, sig, t_eff, g_eff,
                        inpaint=None, channel_cond=None, reference=None, cfg=None, ip_embeds=None):
        """The denoise loop over `sig` (any sigma list ending in 0: the full schedule or a truncated one) for the first B packed latents
        of `lat` [B, S, 64]; sample b is conditioned on prompt b // num_images_per_prompt.  Returns the B denoised latents.
        inpaint: None, or per sample b an (image_latents, noise, mask) triple of [S, 64] tensors made on the current stream (the
        inpainting loop, FluxTransformer2DModel.denoise).  channel_cond: None, or per sample b the [S, in_channels - out_channels] condition
        of a channel-conditioned transformer, set on the context that carries sample b next to its prompt (FLUX.1 Fill / Control).
        reference: None, or per sample b the (ref_latents [S_ref, 64], ref_ids [S_ref, 3]) reference tokens of FLUX.1 Kontext, set on the
        context that carries sample b right after its prompt (an entry may be None: no reference for that sample).
        cfg: None, or (negative_prompt_embeds, negative_pooled_prompt_embeds, negative_text_ids, true_cfg_scale): true classifier-free
        guidance -- one (positive, negative) context pair on one stream, samples one after another (FluxTransformer2DModel.denoise_cfg).
        ip_embeds: None, or per loaded IP-Adapter a [1 or n_prompts, n_img, E] tensor: the image prompt of sample b, set on the context that
        carries it next to its prompt.  With adapters loaded and no image prompt the contexts' image prompts are cleared (the plain model)."""
        tr = self.transformer
        n_prompts = prompt_embeds.shape[0]
        has_ip = bool(tr.ip_adapters())
        if ip_embeds is not None and cfg is not None:
            raise NotImplementedError("an image prompt under true classifier-free guidance is not built")
        if cfg is not None:
            if inpaint is not None or channel_cond is not None:
                raise NotImplementedError("true classifier-free guidance is built for the plain and the reference-token loop only")
            neg_embeds, neg_pooled, neg_ids, scale = cfg
            pos, neg = self._contexts(2)
            main, st, xs = torch.cuda.current_stream(), self._streams[0], []
            for b in range(B):
                pb = min(b // num_images_per_prompt, n_prompts - 1)
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    for ctx, e, p, ids in ((pos, prompt_embeds, pooled_prompt_embeds, text_ids), (neg, neg_embeds, neg_pooled, neg_ids)):
                        ctx.set_condition(e[min(pb, e.shape[0] - 1)], p[min(pb, p.shape[0] - 1)], img_ids, ids)
                        if has_ip:
                            ctx.set_ip_image_embeds(None)
                        if reference is not None and reference[b] is not None:
                            ctx.set_reference_tokens(*reference[b])
                        ctx.set_timesteps(t_eff, g_eff)
                    x = lat[b].contiguous()
                    pos.denoise_cfg(neg, x, sig, scale)
                main.wait_stream(st)
                xs.append(x)
            return xs
        # `images_in_flight` independent images advance together, each on its own stream and engine context (shared
        # weights): the grids of one step are 1.6 - 3.2 rounds of the 256 CUs, and a second image fills those tails.
        G = max(1, min(int(self.images_in_flight), B))
        ctxs = self._contexts(G)
        main = torch.cuda.current_stream()
        xs = []
        for b0 in range(0, B, G):
            group = list(range(b0, min(b0 + G, B)))
            lat_g = []
            for k, b in enumerate(group):
                pb = min(b // num_images_per_prompt, n_prompts - 1)
                st = self._streams[k]
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    ctxs[k].set_condition(prompt_embeds[pb], pooled_prompt_embeds[min(pb, pooled_prompt_embeds.shape[0] - 1)], img_ids, text_ids)
                    if has_ip:
                        ctxs[k].set_ip_image_embeds(None if ip_embeds is None else [e[min(pb, e.shape[0] - 1)] for e in ip_embeds])
                    if channel_cond is not None:
                        ctxs[k].set_channel_condition(channel_cond[b])
                    if reference is not None and reference[b] is not None:
                        ctxs[k].set_reference_tokens(*reference[b])
                    ctxs[k].set_timesteps(t_eff, g_eff)
                    lat_g.append(lat[b].contiguous())
            blend_g = None if inpaint is None else [inpaint[b] for b in group]
            if len(group) == 1:
                with torch.cuda.stream(self._streams[0]):
                    ctxs[0].denoise(lat_g[0], sig, None if blend_g is None else blend_g[0])
            else:
                type(tr).denoise_multi(ctxs[:len(group)], lat_g, sig, self._streams[:len(group)], blend_g)
            for k in range(len(group)):
                main.wait_stream(self._streams[k])
            xs.extend(lat_g)
        return xs

    def _finish(self, xs, h: int, w: int, output_type: str, return_dict: bool):
        """Denoised packed latents -> the pipeline's output (diffusers' `output_type` / `return_dict`)."""
        tr = self.transformer
        outs = []
        for x in xs:
            if output_type == "latent":      # diffusers: packed latents, no unpack
                outs.append(x)
            elif output_type == "vae_input":  # _unpack_latents + (z / scaling_factor + shift_factor), no decode
                outs.append(_OPS.flux_unpack_latents(x, latent_channels(tr.config) // 4, h, w,
                                                     self.vae_scaling_factor, self.vae_shift_factor))
            elif self.vae is None:
                raise _hip.ThinkDiffHipError("no VAE loaded: call with output_type='latent' (packed latents) or "
                                             "'vae_input' (unpacked, scaled decoder input)")
            else:                             # unpack + affine + vae.decode + postprocess, all in td_vae_decode
                outs.append(self.vae.decode_packed(x, h, w, output_type=output_type))
        images = outs if output_type == "pil" else torch.stack(outs)
        if not return_dict:
            return (images,)
        return SimpleNamespace(images=images)
