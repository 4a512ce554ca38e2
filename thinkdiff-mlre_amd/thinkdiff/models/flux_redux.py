"""FLUX.1 Redux: an image turned into FLUX prompt tokens -- the SigLIP tower's hidden states through a two-Linear prior, then several
`[text | image]` streams folded into the one `prompt_embeds` / `pooled_prompt_embeds` pair every FLUX pipeline here takes.

**Parity unpinned.**  `diffusers` is not installed here (tests/test_diffusers_probe.py); what follows is restated from the published diffusers sources
([ext]): `pipelines/flux/pipeline_flux_prior_redux.py` (`FluxPriorReduxPipeline`) and `pipelines/flux/modeling_flux.py` (`ReduxImageEncoder`).  The
CPU restatement the tests run is tests/redux_common.py; the composition's arithmetic is spelled out in include/thinkdiff_hip.h (td_redux_compose_bf16).

    image_latents = image_encoder(feature_extractor.preprocess(image)).last_hidden_state            [B, 729, 1152]   SiglipVisionModel, so400m-patch14-384
    image_embeds  = redux_down(silu(redux_up(image_latents)))                                       [B, 729, 4096]   ReduxImageEncoder
    prompt_embeds = cat([text [B, T, 4096], image_embeds], dim=1) * prompt_embeds_scale[:, None, None];   prompt_embeds = sum(dim=0, keepdim=True)
    pooled        = pooled [B, P] * pooled_prompt_embeds_scale[:, None];                                  pooled        = sum(dim=0, keepdim=True)

B is the number of images of the call: B images give ONE stream of T + 729 rows, each image's tokens under its own scale.  One string prompt is used
for every image, so its embeddings enter the sum B times, each under its scale.

Where this pipeline departs from diffusers, by decision:
  * a tensor `image` is taken as already preprocessed `pixel_values` [B, 3, H, W] (diffusers would rescale and normalise it again);
  * supplied `prompt_embeds` / `pooled_prompt_embeds` are used whether or not text encoders are loaded (diffusers overwrites them with zeros when it
    has none) -- the ThinkDiff case: the aligner's output as the text part, Redux tokens as the image part;
  * `prompt` without text encoders is a ValueError (diffusers warns and drops it);
  * `max_sequence_length` is a keyword (diffusers fixes it to 512).

Downstream the stream is LONGER than a text prompt: create the transformer with room for it,
    FluxPipelineRewritePrompt.from_pretrained(path, max_txt_tokens=512 + 729)          # max_txt_tokens >= T + 729
    image = flux_pipe(**prior(image), height=1024, width=1024).images[0]

Not built: position interpolation (another image size than the tower's), a HIP resize (the bicubic resize stays on the host in PIL), the
SigLIP pooling head, masked or per-region Redux.
"""
import os
from typing import Dict, List, Optional, Union

import torch

from .. import _hip
from .text_encoders import _Base, _random_sd, _read_dir
from .vision_towers import HipSiglipVisionModel, _pad_k, _round64

REDUX_MAX_IMAGES = 16      # include/thinkdiff_hip.h: td_redux_compose_bf16 takes 1 .. 16 streams


class ReduxImageEncoderOutput:
    def __init__(self, image_embeds: torch.Tensor):
        self.image_embeds = image_embeds


class ReduxImageEncoder(_Base):
    """diffusers `ReduxImageEncoder`: redux_down(silu(redux_up(x))), Linear(redux_dim -> 3 x txt_in_features) and back to txt_in_features: two
    td_linear_bf16 calls, the first with the SiLU epilogue.  Widths that are no multiple of the GEMM's k-tile are zero-padded at load."""

    def __init__(self, sd: Dict[str, torch.Tensor], device="cuda"):
        super().__init__(device)
        g = lambda k: self._dev(sd[k])
        up_w, down_w = g("redux_up.weight"), g("redux_down.weight")
        self.redux_dim, self.txt_in_features = up_w.shape[1], down_w.shape[0]
        if up_w.shape[0] != down_w.shape[1]:
            raise ValueError(f"ReduxImageEncoder: redux_up writes {up_w.shape[0]} columns, redux_down reads {down_w.shape[1]}")
        hidden = _round64(up_w.shape[0])           # silu(0) = 0 meets zero columns of redux_down
        self.up_w = torch.zeros(hidden, _round64(self.redux_dim), dtype=torch.bfloat16, device=self.device)
        self.up_w[:up_w.shape[0], :self.redux_dim] = up_w
        self.up_b = torch.zeros(hidden, dtype=torch.bfloat16, device=self.device)
        self.up_b[:up_w.shape[0]] = g("redux_up.bias")
        self.down_w, self.down_b = _pad_k(down_w).contiguous(), g("redux_down.bias")

    @classmethod
    def from_random(cls, redux_dim: int = 1152, txt_in_features: int = 4096, seed: int = 0, device="cuda"):
        """Synthetic prior of the released shape (defaults) drawn on the device."""
        shapes = {"redux_up.weight": (3 * txt_in_features, redux_dim), "redux_up.bias": (3 * txt_in_features,),
                  "redux_down.weight": (txt_in_features, 3 * txt_in_features), "redux_down.bias": (txt_in_features,)}
        return cls(_random_sd(shapes, seed, torch.device(device)), device=device)

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "image_embedder", device="cuda"):
        _cfg, sd = _read_dir(path, subfolder)
        return cls(sd, device=device)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, **_kw) -> ReduxImageEncoderOutput:
        """x [..., redux_dim] bf16 -> .image_embeds [..., txt_in_features]."""
        if x.shape[-1] != self.redux_dim:
            raise _hip.ThinkDiffHipError(f"ReduxImageEncoder: input width {x.shape[-1]}, redux_up reads {self.redux_dim}")
        rows = x.to(self.device, torch.bfloat16).reshape(-1, self.redux_dim).contiguous()
        if self.up_w.shape[1] != self.redux_dim:
            rows = _hip.cast_pad_rows(rows, self.up_w.shape[1])
        y = _hip.linear(_hip.linear(rows, self.up_w, self.up_b, act=_hip.ACT_SILU), self.down_w, self.down_b)
        return ReduxImageEncoderOutput(y.view(*x.shape[:-1], self.txt_in_features))


class ReduxDefaultImageProcessor:
    """What transformers' PIL SigLIP processor does under the released `feature_extractor/preprocessor_config.json`, for a checkpoint directory
    without one: convert to RGB, resize to size x size bicubic (PIL), x 1/255 (in fp64, rounded to fp32), (x - 0.5) / 0.5 in fp32.

    `device=`: the same values computed on that device -- the image's bytes go up in their own mode ("L", "RGB", "RGBA"), the RGB conversion and the
    resize run as td_image_resize_u8 (Pillow's bytes) and the two arithmetic steps as a lookup in the table of their results for the 256 pixel
    values (td_image_lut_chw_f32); `pixel_values` then lives on the device.  Without it nothing changes."""

    def __init__(self, size: int = 384, image_mean: float = 0.5, image_std: float = 0.5, device=None):
        self.size, self.image_mean, self.image_std = int(size), float(image_mean), float(image_std)
        self.device = torch.device(device) if device is not None else None
        self._lut = None

    def _normalize(self, a):
        import numpy as np
        a = (a.astype(np.float64) * (1 / 255)).astype(np.float32)
        return (a - np.float32(self.image_mean)) / np.float32(self.image_std)

    def _device_lut(self):
        import numpy as np
        if self._lut is None:      # the host path's own arithmetic on every pixel value; one row per channel
            row = self._normalize(np.arange(256, dtype=np.uint8))
            self._lut = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(row, (3, 256)))).to(self.device)
        return self._lut

    def preprocess(self, images, **_kw):
        import numpy as np
        from PIL import Image
        out = []
        for im in ([images] if isinstance(images, Image.Image) else list(images)):
            if self.device is not None:
                im = im if im.mode in ("L", "RGB", "RGBA") else im.convert("RGB")
                a = torch.from_numpy(np.ascontiguousarray(np.asarray(im, dtype=np.uint8))).to(self.device)
                a = _hip.image_resize_u8(a, self.size, self.size, int(Image.BICUBIC), out_channels=3)
                out.append(_hip.image_lut_chw_f32(a, self._device_lut()))
                continue
            a = np.asarray(im.convert("RGB").resize((self.size, self.size), resample=Image.BICUBIC))
            a = self._normalize(a)
            out.append(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))))
        return type("BatchFeature", (), {"pixel_values": torch.stack(out)})()

    __call__ = preprocess


class FluxPriorReduxPipelineOutput(dict):
    """Dict-like with exactly the keys `prompt_embeds`, `pooled_prompt_embeds` (so `flux_pipe(**prior(image), ...)` works), attributes too."""
    prompt_embeds = property(lambda self: self["prompt_embeds"])
    pooled_prompt_embeds = property(lambda self: self["pooled_prompt_embeds"])


def _scales(value, B: int, name: str) -> List[float]:
    if isinstance(value, (int, float)):
        return [float(value)] * B
    value = [float(v) for v in value]
    if len(value) != B:
        raise ValueError(f"{name}: {len(value)} scales for {B} images (a float, or one scale per image)")
    return value


class FluxPriorReduxPipelineRewritePrompt:
    """diffusers' `FluxPriorReduxPipeline` on the HIP ops (module docstring: the statements, and where this departs from them).

    `__call__` returns ONE prompt stream for the images of the call: `prompt_embeds` [1, T + n_patches, J] and `pooled_prompt_embeds` [1, P], to be
    handed to any FLUX pipeline of this package -- whose transformer must have been created with `max_txt_tokens >= T + n_patches` (released shapes:
    512 + 729 = 1241):
        flux_pipe = FluxPipelineRewritePrompt.from_pretrained(path, max_txt_tokens=1241)
        images = flux_pipe(**prior(image), num_inference_steps=28).images
    A tensor `image` is taken as already preprocessed `pixel_values` [B, 3, H, W] -- unlike diffusers, which would preprocess it again."""

    pooled_dim = 768            # diffusers' dummy pooled vector (the CLIP-L width) when no text is given

    def __init__(self, image_encoder, feature_extractor, image_embedder, text_encoder=None, tokenizer=None, text_encoder_2=None, tokenizer_2=None):
        self.image_encoder, self.feature_extractor, self.image_embedder = image_encoder, feature_extractor, image_embedder
        self.text_encoder, self.tokenizer, self.text_encoder_2, self.tokenizer_2 = text_encoder, tokenizer, text_encoder_2, tokenizer_2

    # ---- construction --------------------------------------------------------------------------------
    @staticmethod
    def read_parts(path: str) -> dict:
        """What a local FLUX.1-Redux directory holds, read on the host: `image_encoder` and `image_embedder` as (config, state dict),
        `feature_extractor` (transformers' PIL SigLIP processor when feature_extractor/preprocessor_config.json exists, else the built-in defaults)
        and which text-encoder folders are present.  Hub ids cannot be fetched here."""
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path!r} is not a local directory; this build loads FLUX.1 Redux weights from disk only "
                                    "(or use from_random on the tower and the prior for synthetic weights)")
        parts = {"image_encoder": _read_dir(path, "image_encoder"), "image_embedder": _read_dir(path, "image_embedder")}
        fe_dir = os.path.join(path, "feature_extractor")
        if os.path.isfile(os.path.join(fe_dir, "preprocessor_config.json")):
            try:
                from transformers.models.siglip.image_processing_pil_siglip import SiglipImageProcessorPil as Processor
            except ImportError:          # older transformers: the slow processor is the PIL one
                from transformers import SiglipImageProcessor as Processor
            parts["feature_extractor"] = Processor.from_pretrained(fe_dir)
        else:
            parts["feature_extractor"] = ReduxDefaultImageProcessor()
        parts["text_encoder"] = all(os.path.isdir(os.path.join(path, d)) for d in ("text_encoder", "tokenizer"))
        parts["text_encoder_2"] = all(os.path.isdir(os.path.join(path, d)) for d in ("text_encoder_2", "tokenizer_2"))
        return parts

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=torch.bfloat16, device="cuda", **_kw):
        """Local directory in diffusers layout: image_encoder/, image_embedder/, feature_extractor/preprocessor_config.json (optional: the built-in
        defaults apply), text_encoder/ + tokenizer/ and text_encoder_2/ + tokenizer_2/ (optional)."""
        root = pretrained_model_name_or_path
        parts = cls.read_parts(root)
        cfg, sd = parts["image_encoder"]
        cfg = cfg.get("vision_config", cfg)
        if cfg.get("hidden_act", "gelu_pytorch_tanh") != "gelu_pytorch_tanh":
            raise _hip.ThinkDiffHipError(f"SigLIP hidden_act {cfg['hidden_act']!r}: only gelu_pytorch_tanh is implemented")
        enc = {}
        if parts["text_encoder"]:
            from transformers import CLIPTokenizer
            from .text_encoders import HipCLIPTextEncoder
            enc.update(text_encoder=HipCLIPTextEncoder.from_pretrained(root, device=device), tokenizer=CLIPTokenizer.from_pretrained(os.path.join(root, "tokenizer")))
        if parts["text_encoder_2"]:
            from transformers import AutoTokenizer
            from .text_encoders import HipT5Encoder
            enc.update(text_encoder_2=HipT5Encoder.from_pretrained(root, device=device), tokenizer_2=AutoTokenizer.from_pretrained(os.path.join(root, "tokenizer_2")))
        return cls(HipSiglipVisionModel(sd, cfg.get("num_attention_heads", 16), cfg.get("layer_norm_eps", 1e-6), device), parts["feature_extractor"],
                   ReduxImageEncoder(parts["image_embedder"][1], device=device), **enc)

    def to(self, *_a, **_k):
        return self

    # ---- the call ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, image, prompt: Union[str, List[str], None] = None, prompt_2: Union[str, List[str], None] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, pooled_prompt_embeds: Optional[torch.Tensor] = None,
                 prompt_embeds_scale: Union[float, List[float]] = 1.0, pooled_prompt_embeds_scale: Union[float, List[float]] = 1.0,
                 max_sequence_length: int = 512, return_dict: bool = True):
        """image: a PIL image, a list of them, or a tensor [B, 3, H, W] of ALREADY PREPROCESSED pixel_values (unlike diffusers).  B = the number of
        images.  Text part: supplied `prompt_embeds` [1 or B, T, J] with `pooled_prompt_embeds` [1 or B, P]; or `prompt` (a string is used for every
        image) through the loaded text encoders; or neither: `max_sequence_length` zero rows and a zero pooled vector of 768.  Scales: a float or one
        per image.  -> {prompt_embeds [1, T + n_patches, J], pooled_prompt_embeds [1, P]} (a tuple with return_dict=False)."""
        # every refusal comes before any GPU work
        if isinstance(image, torch.Tensor):
            if image.dim() != 4 or image.shape[1] != 3:
                raise ValueError(f"image: a tensor must be preprocessed pixel_values [B, 3, H, W], got {tuple(image.shape)}")
            B = image.shape[0]
        elif isinstance(image, (list, tuple)):
            B = len(image)
        else:
            image, B = [image], 1
        if B < 1 or B > REDUX_MAX_IMAGES:
            raise ValueError(f"image: {B} images in one call, 1 .. {REDUX_MAX_IMAGES} are supported")
        s_embeds = _scales(prompt_embeds_scale, B, "prompt_embeds_scale")
        s_pooled = _scales(pooled_prompt_embeds_scale, B, "pooled_prompt_embeds_scale")
        J = int(self.image_embedder.txt_in_features)
        if (prompt_embeds is None) != (pooled_prompt_embeds is None):
            given, missing = ("prompt_embeds", "pooled_prompt_embeds") if pooled_prompt_embeds is None else ("pooled_prompt_embeds", "prompt_embeds")
            raise ValueError(f"{given} was given without {missing}: supply both or neither")
        if prompt is not None or prompt_2 is not None:
            if prompt_embeds is not None:
                raise ValueError("prompt and prompt_embeds were both given: supply one text source")
            if prompt is None:
                raise ValueError("prompt_2 was given without prompt")
            if None in (self.text_encoder, self.tokenizer, self.text_encoder_2, self.tokenizer_2):
                raise ValueError("prompt was given but no text encoders are loaded (text_encoder / tokenizer / text_encoder_2 / tokenizer_2): "
                                 "pass prompt_embeds and pooled_prompt_embeds, or load the encoders")
            for name, p in (("prompt", prompt), ("prompt_2", prompt_2)):
                if isinstance(p, (list, tuple)) and len(p) not in (1, B):
                    raise ValueError(f"{name}: a batch of {len(p)} prompts for {B} images (a string, or one prompt per image)")
        if prompt_embeds is not None:
            if prompt_embeds.dim() != 3 or pooled_prompt_embeds.dim() != 2:
                raise ValueError(f"prompt_embeds must be [1 or {B}, T, {J}] and pooled_prompt_embeds [1 or {B}, P], got {tuple(prompt_embeds.shape)} and "
                                 f"{tuple(pooled_prompt_embeds.shape)}")
            if prompt_embeds.shape[2] != J:
                raise ValueError(f"prompt_embeds has width {prompt_embeds.shape[2]}, the prior's image tokens have width {J}")
            for name, t in (("prompt_embeds", prompt_embeds), ("pooled_prompt_embeds", pooled_prompt_embeds)):
                if t.shape[0] not in (1, B):
                    raise ValueError(f"{name} has batch {t.shape[0]}, the call has {B} images (batch 1 or {B})")
        if max_sequence_length < 1:
            raise ValueError(f"max_sequence_length={max_sequence_length} must be positive")

        dev = getattr(self.image_encoder, "device", torch.device("cuda"))
        if isinstance(image, torch.Tensor):
            pixel_values = image
        else:
            pixel_values = self.feature_extractor.preprocess(images=list(image), do_resize=True, return_tensors="pt", do_convert_rgb=True).pixel_values
        image_latents = self.image_encoder(pixel_values).last_hidden_state
        image_embeds = self.image_embedder(image_latents).image_embeds.contiguous()                # [B, n_patches, J]
        text = pooled = None
        if prompt is not None:
            text, pooled = self._encode_text(prompt, prompt_2, max_sequence_length, dev)
            if text.shape[2] != J:
                raise ValueError(f"the T5 encoder's width {text.shape[2]} differs from the prior's {J}")
        elif prompt_embeds is not None:
            text = prompt_embeds.to(dev, torch.bfloat16).contiguous()
            pooled = pooled_prompt_embeds.to(dev, torch.bfloat16).contiguous()
        out = _hip.redux_compose(text, image_embeds, s_embeds, T=max_sequence_length)
        pooled_out = _hip.redux_compose(pooled[:, None, :] if pooled is not None else None, None, s_pooled, T=1, D=self.pooled_dim, device=dev)
        result = FluxPriorReduxPipelineOutput(prompt_embeds=out[None], pooled_prompt_embeds=pooled_out)
        return result if return_dict else (result["prompt_embeds"], result["pooled_prompt_embeds"])

    def _encode_text(self, prompt, prompt_2, max_sequence_length: int, dev):
        """[ext] FluxPipeline._get_clip_prompt_embeds / _get_t5_prompt_embeds: (T5 hidden states [b, T, J], CLIP pooler_output [b, P]), b = 1 for a string."""
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        prompt_2 = prompt if prompt_2 is None else ([prompt_2] if isinstance(prompt_2, str) else list(prompt_2))
        if len(prompt_2) != len(prompt):
            raise ValueError(f"prompt has {len(prompt)} entries, prompt_2 {len(prompt_2)}")
        ids = self.tokenizer(prompt, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        pooled = self.text_encoder(ids.to(dev), output_hidden_states=False).pooler_output
        ids = self.tokenizer_2(prompt_2, padding="max_length", max_length=max_sequence_length, truncation=True, return_tensors="pt").input_ids
        text = self.text_encoder_2(ids.to(dev), output_hidden_states=False)[0]
        return text.to(torch.bfloat16).contiguous(), pooled.to(torch.bfloat16).contiguous()
