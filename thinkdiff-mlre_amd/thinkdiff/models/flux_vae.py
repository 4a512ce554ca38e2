"""FLUX VAE decoder on the HIP engine (`td_vae_*`): stands in for `diffusion_pipe.vae` ([ext] diffusers 0.31.0
`AutoencoderKL`) + `VaeImageProcessor.postprocess`; `AutoencoderKLEncoder` (`td_vae_enc_*`) adds the encode path.  Parameter names = diffusers state dict."""
import ctypes
import dataclasses
import glob
import json
import os
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import torch

from .. import _hip
from ..ops import register as _register_ops

_OPS = _register_ops()      # torch.ops.thinkdiff_hip (the uint8 decode goes through it)


@dataclasses.dataclass
class AutoencoderKLConfig:
    """Decoder-side keys of [ext] FLUX.1-dev vae/config.json."""
    latent_channels: int = 16
    out_channels: int = 3
    block_out_channels: Sequence[int] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.3611
    shift_factor: float = 0.1159


class AutoencoderKLDecoder:
    dtype = torch.bfloat16

    def __init__(self, config: AutoencoderKLConfig = None, max_latent_size=(128, 128), device="cuda"):
        self.config = config or AutoencoderKLConfig()
        c = self.config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _hip.ThinkDiffHipError("AutoencoderKLDecoder runs on the MI355X HIP engine only (device='cuda')")
        self._L = _hip.lib()
        boc = list(c.block_out_channels) + [0] * (4 - len(c.block_out_channels))
        cc = _hip.TdVaeConfig(c.latent_channels, c.out_channels, len(c.block_out_channels), (ctypes.c_int * 4)(*boc),
                              c.layers_per_block, c.norm_num_groups)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(self._L.td_vae_create(ctypes.byref(cc), max_latent_size[0], max_latent_size[1], ctypes.byref(h)))
        self._h = h
        self.upscale = 2 ** (len(c.block_out_channels) - 1)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.td_vae_destroy(h)

    def param_table(self) -> Dict[str, int]:
        buf, cnt, out = ctypes.create_string_buffer(256), ctypes.c_int64(), {}
        for i in range(self._L.td_vae_num_params(self._h)):
            _hip.check(self._L.td_vae_param_info(self._h, i, buf, 256, ctypes.byref(cnt)))
            out[buf.value.decode()] = cnt.value
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        table = self.param_table()
        missing = [k for k in table if k not in sd]
        if strict and missing:
            raise KeyError(f"AutoencoderKLDecoder.load_state_dict: missing {missing[:4]}..")
        for name, t in sd.items():
            if name in table:     # encoder.* / quant_conv.* keys of a full checkpoint are ignored
                d = t.to(device=self.device, dtype=torch.bfloat16).contiguous()
                _hip.check(self._L.td_vae_load_param(self._h, name.encode(), _hip.ptr(d), d.numel(), _hip.stream_ptr()))
                torch.cuda.current_stream().synchronize()
        return missing

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "vae", **kw):
        from safetensors import safe_open
        root = os.path.join(path, subfolder) if os.path.isdir(os.path.join(path, subfolder)) else path
        with open(os.path.join(root, "config.json")) as fh:
            raw = json.load(fh)
        fields = {f.name for f in dataclasses.fields(AutoencoderKLConfig)}
        m = cls(AutoencoderKLConfig(**{k: v for k, v in raw.items() if k in fields}), **kw)
        seen = set()
        for fn in sorted(glob.glob(os.path.join(root, "*.safetensors"))):
            with safe_open(fn, framework="pt") as fh:
                part = {k: fh.get_tensor(k) for k in fh.keys()}
            m.load_state_dict(part, strict=False)
            seen.update(part)
        # every decoder tensor must have arrived: an older VAE export (attention weights named query/key/value/proj_attn)
        # would otherwise leave parts of the weight arena uninitialised and decode garbage without an error
        missing = [k for k in m.param_table() if k not in seen]
        if missing:
            raise KeyError(f"VAE checkpoint at {root} lacks {len(missing)} decoder tensors, e.g. {missing[:3]}")
        return m

    def init_random(self, seed: int = 0, std: float = 0.0):
        """Seeded synthetic decoder; std <= 0 (default): 1 / sqrt(fan_in) weights, so decoded images have contrast."""
        _hip.check(self._L.td_vae_init_random(self._h, seed, std, _hip.stream_ptr()))
        return self

    @torch.no_grad()
    def decode_packed(self, packed_latents, h: int, w: int, output_type: str = "pil"):
        """packed [(h/2)(w/2), 4C] bf16 (the denoised FLUX latents) -> image.  output_type: "pil" | "np" (uint8 HWC)
        | "pt" (bf16 [3,H,W], the raw vae.decode output)."""
        x = packed_latents.to(self.device, torch.bfloat16).contiguous()
        H, W = h * self.upscale, w * self.upscale
        if output_type == "pt":
            chw = torch.empty(3, H, W, dtype=torch.bfloat16, device=self.device)
            _hip.check(self._L.td_vae_decode(self._h, _hip.ptr(x), h, w, self.config.scaling_factor, self.config.shift_factor, None, _hip.ptr(chw), _hip.stream_ptr()))
            return chw
        u8 = _OPS.vae_decode_u8(int(self._h.value), x, int(h), int(w), float(self.config.scaling_factor), float(self.config.shift_factor))
        if output_type == "np":
            return u8
        from PIL import Image
        return Image.fromarray(u8.cpu().numpy())


class AutoencoderKLEncoder:
    """FLUX VAE encoder on the HIP engine (`td_vae_enc_*`): stands in for [ext] diffusers 0.31.0 `AutoencoderKL.encoder`
    (double_z, no quant_conv, mid-block attention) with `VaeImageProcessor.preprocess`'s normalisation fused in front.
    Configured by the same `AutoencoderKLConfig` as the decoder; parameter names = diffusers state dict (`encoder.*`)."""
    dtype = torch.bfloat16

    def __init__(self, config: AutoencoderKLConfig = None, max_image_size=(1024, 1024), device="cuda"):
        self.config = config or AutoencoderKLConfig()
        c = self.config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _hip.ThinkDiffHipError("AutoencoderKLEncoder runs on the MI355X HIP engine only (device='cuda')")
        self._L = _hip.lib()
        boc = list(c.block_out_channels) + [0] * (4 - len(c.block_out_channels))
        cc = _hip.TdVaeConfig(c.latent_channels, c.out_channels, len(c.block_out_channels), (ctypes.c_int * 4)(*boc),
                              c.layers_per_block, c.norm_num_groups)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(self._L.td_vae_enc_create(ctypes.byref(cc), max_image_size[0], max_image_size[1], ctypes.byref(h)))
        self._h = h
        self.max_image_size = (int(max_image_size[0]), int(max_image_size[1]))      # capacity: H * W <= their product
        self.downscale = 2 ** (len(c.block_out_channels) - 1)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.td_vae_enc_destroy(h)

    def param_table(self) -> Dict[str, int]:
        buf, cnt, out = ctypes.create_string_buffer(256), ctypes.c_int64(), {}
        for i in range(self._L.td_vae_enc_num_params(self._h)):
            _hip.check(self._L.td_vae_enc_param_info(self._h, i, buf, 256, ctypes.byref(cnt)))
            out[buf.value.decode()] = cnt.value
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        table = self.param_table()
        missing = [k for k in table if k not in sd]
        if strict and missing:
            raise KeyError(f"AutoencoderKLEncoder.load_state_dict: missing {missing[:4]}..")
        for name, t in sd.items():
            if name in table:     # decoder.* keys of a full checkpoint are the decoder's
                d = t.to(device=self.device, dtype=torch.bfloat16).contiguous()
                _hip.check(self._L.td_vae_enc_load_param(self._h, name.encode(), _hip.ptr(d), d.numel(), _hip.stream_ptr()))
                torch.cuda.current_stream().synchronize()
        return missing

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "vae", **kw):
        """Reads the `encoder.*` tensors of a diffusers-layout VAE folder; a checkpoint that lacks any of them is refused (KeyError)."""
        from safetensors import safe_open
        root = os.path.join(path, subfolder) if os.path.isdir(os.path.join(path, subfolder)) else path
        with open(os.path.join(root, "config.json")) as fh:
            raw = json.load(fh)
        fields = {f.name for f in dataclasses.fields(AutoencoderKLConfig)}
        m = cls(AutoencoderKLConfig(**{k: v for k, v in raw.items() if k in fields}), **kw)
        table, seen = m.param_table(), set()
        for fn in sorted(glob.glob(os.path.join(root, "*.safetensors"))):
            with safe_open(fn, framework="pt") as fh:
                part = {k: fh.get_tensor(k) for k in fh.keys() if k in table}
            m.load_state_dict(part, strict=False)
            seen.update(part)
        missing = [k for k in table if k not in seen]
        if missing:
            raise KeyError(f"VAE checkpoint at {root} lacks {len(missing)} encoder tensors, e.g. {missing[:3]}")
        return m

    def init_random(self, seed: int = 0, std: float = 0.0):
        """Seeded synthetic encoder; std <= 0 (default): 1 / sqrt(fan_in) weights."""
        _hip.check(self._L.td_vae_enc_init_random(self._h, seed, std, _hip.stream_ptr()))
        return self

    @torch.no_grad()
    def encode_moments(self, image: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One image -> the posterior's parameters [h*w, 2C] bf16 (NHWC rows: mean | logvar), h = H / 8 for the FLUX.1 VAE.
        image: uint8 [H, W, 3] (PIL layout, 0..255) or float [3, H, W] in [0, 1]; `VaeImageProcessor.preprocess`'s 2x - 1 and the
        bf16 cast happen on the GPU.  H, W: multiples of 16 within the capacity given at construction.
        mask (uint8 or float32 [H, W]): encode FLUX.1 Fill's masked image instead, image * (1 - binarize(mask)) taken in fp32 before the
        bf16 cast, inside the same image-in kernel (td_vae_encode_masked)."""
        if image.dtype == torch.uint8:
            H, W = int(image.shape[0]), int(image.shape[1])
        else:
            image = image.float()
            H, W = int(image.shape[1]), int(image.shape[2])
        x = image.to(self.device).contiguous()
        if mask is not None:
            return _OPS.vae_encode_moments_masked(int(self._h.value), x, mask.to(self.device).contiguous(), H, W)
        h, w, mc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _hip.check(self._L.td_vae_enc_output_shape(self._h, H, W, ctypes.byref(h), ctypes.byref(w), ctypes.byref(mc)))
        mom = torch.empty(h.value * w.value, mc.value, dtype=torch.bfloat16, device=self.device)
        fmt = _hip.IMAGE_U8_HWC if x.dtype == torch.uint8 else _hip.IMAGE_F32_CHW
        _hip.check(self._L.td_vae_encode(self._h, _hip.ptr(x), fmt, H, W, _hip.ptr(mom), _hip.stream_ptr()))
        return mom


class DiagonalGaussianDistribution:
    """[ext] diffusers vae.py DiagonalGaussianDistribution over the encoder's moments: .mean / .logvar / .std are [B, C, h, w]
    (NCHW, as in diffusers; logvar clamped to [-30, 20]).  `moments` is the list of per-image [h*w, 2C] rows td_vae_encode writes;
    `sample` / `mode` and the pipeline's fused form (`packed_latents`) read those rows directly."""

    def __init__(self, moments, h: int, w: int):
        self.moments, self.h, self.w = list(moments), int(h), int(w)
        self.C = self.moments[0].shape[1] // 2

    def _nchw(self, lo):
        return torch.stack([m.view(self.h, self.w, 2 * self.C)[..., lo:lo + self.C].permute(2, 0, 1) for m in self.moments])

    @property
    def mean(self):
        return self._nchw(0)

    @property
    def logvar(self):
        return torch.clamp(self._nchw(self.C), -30.0, 20.0)

    @property
    def std(self):
        return torch.exp(0.5 * self.logvar)

    def packed_latents(self, i: int, eps=None, noise=None, sigma: float = 0.0, scaling_factor: float = 1.0, shift_factor: float = 0.0):
        """Image i -> packed FLUX latents [(h/2)(w/2), 4C]: sample (eps [C,h,w] bf16) or mode (eps None), (z - shift) * scaling, and
        scale_noise at sigma (noise None: none) -- td_vae_latents_from_moments, with the bf16 rounding points of the torch statements."""
        return _OPS.vae_latents_from_moments(self.moments[i], eps, noise, float(sigma), float(scaling_factor), float(shift_factor), self.h, self.w)

    def _unpacked(self, eps):
        return torch.stack([_OPS.flux_unpack_latents(self.packed_latents(i, None if eps is None else eps[i].contiguous()), self.C, self.h, self.w, 1.0, 0.0)
                            for i in range(len(self.moments))])

    def sample(self, generator=None):
        """mean + std * eps with eps = randn([B, C, h, w], generator, bf16) on the moments' device (randn_tensor's draw)."""
        eps = torch.randn((len(self.moments), self.C, self.h, self.w), generator=generator, device=self.moments[0].device, dtype=torch.bfloat16)
        return self._unpacked(eps)

    def mode(self):
        return self._unpacked(None)


class AutoencoderKL:
    """Encoder + decoder: `encode(x).latent_dist` as in diffusers, and the decoder's `decode_packed`."""
    dtype = torch.bfloat16

    def __init__(self, encoder: AutoencoderKLEncoder, decoder: AutoencoderKLDecoder):
        self.encoder, self.decoder = encoder, decoder
        self.config = decoder.config

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "vae", max_latent_size=(128, 128), max_image_size=(1024, 1024), device="cuda"):
        return cls(AutoencoderKLEncoder.from_pretrained(path, subfolder, max_image_size=max_image_size, device=device),
                   AutoencoderKLDecoder.from_pretrained(path, subfolder, max_latent_size=max_latent_size, device=device))

    @torch.no_grad()
    def encode(self, x, return_dict: bool = True):
        """x: float [B, 3, H, W] in [0, 1] or uint8 [B, H, W, 3] -- the image BEFORE `VaeImageProcessor.preprocess`, whose 2x - 1
        runs inside the encoder (diffusers: `vae.encode(image_processor.preprocess(image))`)."""
        moments = [self.encoder.encode_moments(x[i]) for i in range(x.shape[0])]
        H = x.shape[1] if x.dtype == torch.uint8 else x.shape[2]
        W = x.shape[2] if x.dtype == torch.uint8 else x.shape[3]
        dist = DiagonalGaussianDistribution(moments, H // self.encoder.downscale, W // self.encoder.downscale)
        return SimpleNamespace(latent_dist=dist) if return_dict else (dist,)

    def decode_packed(self, packed_latents, h: int, w: int, output_type: str = "pil"):
        return self.decoder.decode_packed(packed_latents, h, w, output_type=output_type)
