"""Vision towers upstream of the aligner, on the HIP ops.

* `HipBlip2VisionModel` -- EVA-ViT-g as wrapped by transformers `Blip2VisionModel` (39 layers, D 1408, 16 heads x 88,
  MLP 6144, 14x14 patches of a 224^2 image -> 257 tokens): `self.vision_model(pixel_values)[0]` in
  reference thinkdiff/models/blip_vision_t5_decoder.py:611-618.
* `HipQwen2VisionTransformer` -- the Qwen2-VL ViT (32 blocks, D 1280, 16 heads x 80, 2-D rotary, full attention per
  image, 2x2 patch merger) that vLLM runs inside `self.mllama.generate` (mllama_vllm_t5_embed_decoder_2.py:1083-1089);
  oracle = transformers `Qwen2VisionTransformerPretrainedModel`.
* `HipSiglipVisionModel` -- the SigLIP so400m ViT as transformers `SiglipVisionModel` (27 layers, D 1152, 16 heads x 72, MLP 4304, 14x14 patches of a
  384^2 image -> 729 tokens, no class token): the image encoder of FLUX.1 Redux (thinkdiff/models/flux_redux.py), which reads `last_hidden_state`.

Heads of width 88 / 80 are zero-padded to the attention kernel's 128 columns inside the fused projection weights
(built once at load): q.k is unchanged by zero columns and the padded value columns meet zero rows of the output
projection.  GEMM K must be a multiple of 64, so the patch operands (588 / 1176 wide) are zero-padded to 640 / 1216; SigLIP's MLP width (4304) is padded the
same way to 4352 (zero fc1 rows and bias give gelu(0) = 0 against zero fc2 columns).
"""
from typing import Dict, Sequence

import torch

from .. import _hip
from .text_encoders import HP, _Base, _EncoderOutput, _pad_heads_cols, _pad_heads_rows, _pad_heads_vec, _random_sd, _read_dir


def _round64(k: int) -> int:
    return (k + 63) // 64 * 64


def _pad_k(w: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(w.shape[0], _round64(w.shape[1]), dtype=w.dtype, device=w.device)
    out[:, :w.shape[1]] = w
    return out


class HipBlip2VisionModel(_Base):
    def __init__(self, sd: Dict[str, torch.Tensor], num_heads: int = 16, patch_size: int = 14, eps: float = 1e-6, device="cuda"):
        super().__init__(device)
        pre = "vision_model." if "vision_model.embeddings.class_embedding" in sd else ""
        g = lambda k: self._dev(sd[pre + k])
        self.cls = g("embeddings.class_embedding").view(1, -1)
        self.pos = g("embeddings.position_embedding").view(-1, self.cls.shape[1])
        self.D = self.cls.shape[1]
        self.H, self.hd, self.p, self.eps = num_heads, self.D // num_heads, patch_size, eps
        self.patch_w = _pad_k(g("embeddings.patch_embedding.weight").view(self.D, -1)).contiguous()
        self.patch_b = g("embeddings.patch_embedding.bias")
        self.layers = []
        i = 0
        while f"{pre}encoder.layers.{i}.self_attn.qkv.weight" in sd:
            p = f"encoder.layers.{i}."
            w = g(p + "self_attn.qkv.weight")                                   # rows ordered [3][H][hd]
            if (pre + p + "self_attn.qkv.bias") in sd:
                b = g(p + "self_attn.qkv.bias")
            elif (pre + p + "self_attn.q_bias") in sd:                          # on-disk BLIP-2 checkpoints: k has no bias
                b = torch.cat([g(p + "self_attn.q_bias"), torch.zeros(self.D, dtype=torch.bfloat16, device=self.device), g(p + "self_attn.v_bias")])
            else:
                b = torch.zeros(3 * self.D, dtype=torch.bfloat16, device=self.device)
            self.layers.append(dict(
                ln1w=g(p + "layer_norm1.weight"), ln1b=g(p + "layer_norm1.bias"),
                qkv_w=_pad_heads_rows(w, 3 * self.H, self.hd).contiguous(), qkv_b=_pad_heads_vec(b, 3 * self.H, self.hd, self.device),
                o_w=_pad_heads_cols(g(p + "self_attn.projection.weight"), self.H, self.hd).contiguous(), o_b=g(p + "self_attn.projection.bias"),
                ln2w=g(p + "layer_norm2.weight"), ln2b=g(p + "layer_norm2.bias"),
                fc1_w=g(p + "mlp.fc1.weight"), fc1_b=g(p + "mlp.fc1.bias"), fc2_w=g(p + "mlp.fc2.weight"), fc2_b=g(p + "mlp.fc2.bias")))
            i += 1
        self.post_w, self.post_b = g("post_layernorm.weight"), g("post_layernorm.bias")

    @classmethod
    def from_random(cls, hidden=1408, num_layers=39, num_heads=16, intermediate=6144, image_size=224, patch_size=14, seed=0, device="cuda"):
        """Synthetic EVA-ViT-g-shaped tower (defaults = Salesforce/blip2-flan-t5-xxl vision_config) drawn on the device."""
        n_pos = (image_size // patch_size) ** 2 + 1
        shapes = {"embeddings.class_embedding": (1, 1, hidden), "embeddings.position_embedding": (1, n_pos, hidden),
                  "embeddings.patch_embedding.weight": (hidden, 3, patch_size, patch_size), "embeddings.patch_embedding.bias": (hidden,),
                  "post_layernorm.weight": (hidden,), "post_layernorm.bias": (hidden,)}
        for i in range(num_layers):
            p = f"encoder.layers.{i}."
            shapes.update({p + "self_attn.qkv.weight": (3 * hidden, hidden), p + "self_attn.qkv.bias": (3 * hidden,),
                           p + "self_attn.projection.weight": (hidden, hidden), p + "self_attn.projection.bias": (hidden,),
                           p + "layer_norm1.weight": (hidden,), p + "layer_norm1.bias": (hidden,), p + "layer_norm2.weight": (hidden,),
                           p + "layer_norm2.bias": (hidden,), p + "mlp.fc1.weight": (intermediate, hidden), p + "mlp.fc1.bias": (intermediate,),
                           p + "mlp.fc2.weight": (hidden, intermediate), p + "mlp.fc2.bias": (hidden,)})
        return cls(_random_sd(shapes, seed, torch.device(device)), num_heads, patch_size, device=device)

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "", device="cuda"):
        cfg, sd = _read_dir(path, subfolder)
        cfg = cfg.get("vision_config", cfg)
        return cls(sd, cfg.get("num_attention_heads", 16), cfg.get("patch_size", 14), cfg.get("layer_norm_eps", 1e-6), device)

    @torch.no_grad()
    def __call__(self, pixel_values: torch.Tensor, **_kw):
        """pixel_values [B,3,224,224] (fp32 or bf16) -> ([B,257,D] post-layernormed hidden states, pooled [B,D])."""
        outs = []
        for img in pixel_values:
            img = img.to(self.device)
            img = img.contiguous() if img.dtype in (torch.float32, torch.bfloat16) else img.float().contiguous()
            patches = _hip.patchify(img, self.p, self.patch_w.shape[1])
            n = patches.shape[0]
            if n + 1 != self.pos.shape[0]:
                raise _hip.ThinkDiffHipError(f"image gives {n} patches; position table holds {self.pos.shape[0] - 1} (interpolation is not implemented)")
            h = torch.empty(n + 1, self.D, dtype=torch.bfloat16, device=self.device)
            h[0] = self.cls[0]
            _hip.linear(patches, self.patch_w, self.patch_b, out=h[1:])
            h = _hip.add_rows(h, self.pos)
            for L in self.layers:
                x = _hip.layernorm(h, L["ln1w"], L["ln1b"], self.eps)
                a = _hip.attention_padded(_hip.linear(x, L["qkv_w"], L["qkv_b"]), self.H, self.hd ** -0.5)
                h = _hip.linear(a, L["o_w"], L["o_b"], res=h)
                x = _hip.layernorm(h, L["ln2w"], L["ln2b"], self.eps)
                h = _hip.linear(_hip.linear(x, L["fc1_w"], L["fc1_b"], act=_hip.ACT_GELU_ERF), L["fc2_w"], L["fc2_b"], res=h)
            outs.append(_hip.layernorm(h, self.post_w, self.post_b, self.eps))
        hs = torch.stack(outs)
        pooled = torch.stack([_hip.layernorm(o[:1].contiguous(), self.post_w, self.post_b, self.eps)[0] for o in outs])
        return _EncoderOutput((hs, pooled))


def siglip_padded_weights(sd: Dict[str, torch.Tensor], num_heads: int) -> dict:
    """The operands `HipSiglipVisionModel` runs on, built from a transformers SigLIP vision state dict (with or without the `vision_model.`
    prefix; `head.*` ignored) in the dtype and on the device of its tensors -- plain tensor surgery, so it is checkable on the host in fp32:
      patch_w [D, round64(3 p p)], pos [n_patches, D];  per layer  qkv_w [3 H 128, Dk] / qkv_b (q | k | v, every head zero-padded to 128 columns),
      o_w [D, H 128], fc1_w [Ip, Dk] / fc1_b [Ip], fc2_w [D, Ip]     with Dk = round64(D), Ip = round64(intermediate): zero padding throughout."""
    pre = "vision_model." if "vision_model.embeddings.patch_embedding.weight" in sd else ""
    if pre + "embeddings.patch_embedding.weight" not in sd:
        raise KeyError("embeddings.patch_embedding.weight not found in the state dict (with or without the vision_model. prefix)")
    g = lambda k: sd[pre + k]
    w = g("embeddings.patch_embedding.weight")
    D, H = w.shape[0], num_heads
    hd = D // H
    if hd * H != D or hd > HP:
        raise ValueError(f"SigLIP width {D} does not split into {H} heads of at most {HP} columns")

    def vec(b):      # _pad_heads_vec in b's own dtype (that one always answers in bf16)
        o = torch.zeros(H * HP, dtype=b.dtype, device=b.device)
        o.view(H, HP)[:, :hd] = b.view(H, hd)
        return o

    out = dict(D=D, H=H, hd=hd, patch=w.shape[-1], patch_w=_pad_k(w.reshape(D, -1)).contiguous(), patch_b=g("embeddings.patch_embedding.bias"),
               pos=g("embeddings.position_embedding.weight").contiguous(), post_w=g("post_layernorm.weight"), post_b=g("post_layernorm.bias"), layers=[])
    i = 0
    while f"{pre}encoder.layers.{i}.self_attn.q_proj.weight" in sd:
        p = f"encoder.layers.{i}."
        fc1_w, fc1_b, fc2_w = g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias"), g(p + "mlp.fc2.weight")
        Ip = _round64(fc1_w.shape[0])
        fc1_wp = torch.zeros(Ip, _round64(D), dtype=fc1_w.dtype, device=fc1_w.device)
        fc1_wp[:fc1_w.shape[0], :D] = fc1_w
        fc1_bp = torch.zeros(Ip, dtype=fc1_b.dtype, device=fc1_b.device)
        fc1_bp[:fc1_b.shape[0]] = fc1_b
        out["layers"].append(dict(
            ln1w=g(p + "layer_norm1.weight"), ln1b=g(p + "layer_norm1.bias"),
            qkv_w=_pad_k(torch.cat([_pad_heads_rows(g(p + f"self_attn.{n}_proj.weight"), H, hd) for n in "qkv"])).contiguous(),
            qkv_b=torch.cat([vec(g(p + f"self_attn.{n}_proj.bias")) for n in "qkv"]).contiguous(),
            o_w=_pad_heads_cols(g(p + "self_attn.out_proj.weight"), H, hd).contiguous(), o_b=g(p + "self_attn.out_proj.bias"),
            ln2w=g(p + "layer_norm2.weight"), ln2b=g(p + "layer_norm2.bias"),
            fc1_w=fc1_wp, fc1_b=fc1_bp, fc2_w=_pad_k(fc2_w).contiguous(), fc2_b=g(p + "mlp.fc2.bias")))
        i += 1
    return out


class HipSiglipVisionModel(_Base):
    """transformers `SiglipVisionModel` up to `last_hidden_state` (no class token, learned position table, LayerNorm with affine, gelu_pytorch_tanh
    MLP, attention scale head_dim^-0.5, post_layernorm).  The pooling head (`head.*`) is not built: FLUX.1 Redux reads the hidden states."""

    def __init__(self, sd: Dict[str, torch.Tensor], num_heads: int = 16, eps: float = 1e-6, device="cuda"):
        super().__init__(device)
        sd = {k: self._dev(v) for k, v in sd.items() if ".head." not in "." + k}
        P = siglip_padded_weights(sd, num_heads)
        self.D, self.H, self.hd, self.p, self.eps = P["D"], P["H"], P["hd"], P["patch"], eps
        self.Dk = _round64(self.D)
        self.patch_w, self.patch_b, self.pos = P["patch_w"], P["patch_b"], P["pos"]
        self.layers, self.post_w, self.post_b = P["layers"], P["post_w"], P["post_b"]

    @classmethod
    def from_random(cls, hidden=1152, num_layers=27, num_heads=16, intermediate=4304, image_size=384, patch_size=14, seed=0, device="cuda"):
        """Synthetic so400m-shaped tower (defaults = google/siglip-so400m-patch14-384 vision_config: 729 tokens) drawn on the device."""
        shapes = {"embeddings.patch_embedding.weight": (hidden, 3, patch_size, patch_size), "embeddings.patch_embedding.bias": (hidden,),
                  "embeddings.position_embedding.weight": ((image_size // patch_size) ** 2, hidden),
                  "post_layernorm.weight": (hidden,), "post_layernorm.bias": (hidden,)}
        for i in range(num_layers):
            p = f"encoder.layers.{i}."
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                shapes.update({p + f"self_attn.{n}.weight": (hidden, hidden), p + f"self_attn.{n}.bias": (hidden,)})
            shapes.update({p + "layer_norm1.weight": (hidden,), p + "layer_norm1.bias": (hidden,), p + "layer_norm2.weight": (hidden,),
                           p + "layer_norm2.bias": (hidden,), p + "mlp.fc1.weight": (intermediate, hidden), p + "mlp.fc1.bias": (intermediate,),
                           p + "mlp.fc2.weight": (hidden, intermediate), p + "mlp.fc2.bias": (hidden,)})
        return cls(_random_sd(shapes, seed, torch.device(device)), num_heads, device=device)

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "image_encoder", device="cuda"):
        cfg, sd = _read_dir(path, subfolder)
        cfg = cfg.get("vision_config", cfg)
        if cfg.get("hidden_act", "gelu_pytorch_tanh") != "gelu_pytorch_tanh":
            raise _hip.ThinkDiffHipError(f"SigLIP hidden_act {cfg['hidden_act']!r}: only gelu_pytorch_tanh is implemented")
        return cls(sd, cfg.get("num_attention_heads", 16), cfg.get("layer_norm_eps", 1e-6), device)

    @torch.no_grad()
    def __call__(self, pixel_values: torch.Tensor, **_kw):
        """pixel_values [B,3,H,W] (fp32 or bf16, already resized and normalised) -> last_hidden_state [B, (H/p)(W/p), D] after post_layernorm;
        `pooler_output` is None."""
        outs = []
        for img in pixel_values:
            img = img.to(self.device)
            img = img.contiguous() if img.dtype in (torch.float32, torch.bfloat16) else img.float().contiguous()
            patches = _hip.patchify(img, self.p, self.patch_w.shape[1])
            n = patches.shape[0]
            if n != self.pos.shape[0]:
                raise _hip.ThinkDiffHipError(f"image gives {n} patches; position table holds {self.pos.shape[0]} (interpolation is not implemented)")
            h = _hip.add_rows(_hip.linear(patches, self.patch_w, self.patch_b), self.pos)
            # GEMM K is a multiple of 64: a width that is not (tests) is normalised into the leading columns of a zeroed operand
            x = torch.zeros(n, self.Dk, dtype=torch.bfloat16, device=self.device) if self.Dk != self.D else None
            xv = x[:, :self.D] if x is not None else None
            for L in self.layers:
                y = _hip.layernorm(h, L["ln1w"], L["ln1b"], self.eps, out=xv)
                a = _hip.attention_padded(_hip.linear(y if x is None else x, L["qkv_w"], L["qkv_b"]), self.H, self.hd ** -0.5)
                h = _hip.linear(a, L["o_w"], L["o_b"], res=h)
                y = _hip.layernorm(h, L["ln2w"], L["ln2b"], self.eps, out=xv)
                h = _hip.linear(_hip.linear(y if x is None else x, L["fc1_w"], L["fc1_b"], act=_hip.ACT_GELU_TANH), L["fc2_w"], L["fc2_b"], res=h)
            outs.append(_hip.layernorm(h, self.post_w, self.post_b, self.eps))
        return _EncoderOutput((torch.stack(outs), None))


def vision_position_ids(grid_thw: Sequence[Sequence[int]], merge: int = 2) -> torch.Tensor:
    """[S, 2] (row, column) of every patch in the processor's merge-window order: patches are emitted
    block-by-block (merge x merge neighbours adjacent), frames repeat the grid ([ext] Qwen2-VL rot_pos_emb)."""
    out = []
    for t, h, w in grid_thw:
        t, h, w = int(t), int(h), int(w)
        hp = torch.arange(h)[:, None].expand(h, w).reshape(h // merge, merge, w // merge, merge).permute(0, 2, 1, 3).flatten()
        wp = torch.arange(w)[None, :].expand(h, w).reshape(h // merge, merge, w // merge, merge).permute(0, 2, 1, 3).flatten()
        out.append(torch.stack([hp, wp], -1).repeat(t, 1))
    return torch.cat(out)


class HipQwen2VisionTransformer(_Base):
    def __init__(self, sd: Dict[str, torch.Tensor], num_heads: int = 16, spatial_merge_size: int = 2, hidden_act: str = "quick_gelu",
                 rope_theta: float = 10000.0, device="cuda"):
        super().__init__(device)
        pre = next((p for p in ("model.visual.", "visual.", "") if (p + "patch_embed.proj.weight") in sd), None)
        if pre is None:
            raise KeyError("patch_embed.proj.weight not found in the state dict")
        g = lambda k: self._dev(sd[pre + k])
        w = g("patch_embed.proj.weight")
        self.D = w.shape[0]
        self.K_in = w[0].numel()
        self.patch_w = _pad_k(w.view(self.D, -1)).contiguous()
        self.H, self.hd, self.merge, self.theta = num_heads, self.D // num_heads, spatial_merge_size, rope_theta
        self.act = {"quick_gelu": _hip.ACT_QUICK_GELU, "gelu": _hip.ACT_GELU_ERF, "gelu_pytorch_tanh": _hip.ACT_GELU_TANH, "silu": _hip.ACT_SILU}[hidden_act]
        self.layers = []
        i = 0
        while f"{pre}blocks.{i}.attn.qkv.weight" in sd:
            p = f"blocks.{i}."
            self.layers.append(dict(
                ln1w=g(p + "norm1.weight"), ln1b=g(p + "norm1.bias"),
                qkv_w=_pad_heads_rows(g(p + "attn.qkv.weight"), 3 * self.H, self.hd).contiguous(),
                qkv_b=_pad_heads_vec(g(p + "attn.qkv.bias"), 3 * self.H, self.hd, self.device),
                o_w=_pad_heads_cols(g(p + "attn.proj.weight"), self.H, self.hd).contiguous(), o_b=g(p + "attn.proj.bias"),
                ln2w=g(p + "norm2.weight"), ln2b=g(p + "norm2.bias"),
                fc1_w=g(p + "mlp.fc1.weight"), fc1_b=g(p + "mlp.fc1.bias"), fc2_w=g(p + "mlp.fc2.weight"), fc2_b=g(p + "mlp.fc2.bias")))
            i += 1
        self.lnq_w, self.lnq_b = g("merger.ln_q.weight"), g("merger.ln_q.bias")
        self.m0_w, self.m0_b = g("merger.mlp.0.weight"), g("merger.mlp.0.bias")
        self.m2_w, self.m2_b = g("merger.mlp.2.weight"), g("merger.mlp.2.bias")

    @property
    def padded_patch_dim(self) -> int:
        """Columns of the patch-embedding GEMM operand (C T p p rounded up to the k-tile)."""
        return self.patch_w.shape[1]

    @classmethod
    def from_random(cls, embed_dim=1280, depth=32, num_heads=16, mlp_ratio=4, out_hidden=3584, patch_size=14, temporal_patch_size=2,
                    merge=2, seed=0, device="cuda"):
        """Synthetic Qwen2-VL-7B-shaped tower (defaults; the 2B model has out_hidden 1536) drawn on the device."""
        shapes = {"patch_embed.proj.weight": (embed_dim, 3, temporal_patch_size, patch_size, patch_size),
                  "merger.ln_q.weight": (embed_dim,), "merger.ln_q.bias": (embed_dim,),
                  "merger.mlp.0.weight": (embed_dim * merge * merge, embed_dim * merge * merge), "merger.mlp.0.bias": (embed_dim * merge * merge,),
                  "merger.mlp.2.weight": (out_hidden, embed_dim * merge * merge), "merger.mlp.2.bias": (out_hidden,)}
        for i in range(depth):
            p = f"blocks.{i}."
            shapes.update({p + "attn.qkv.weight": (3 * embed_dim, embed_dim), p + "attn.qkv.bias": (3 * embed_dim,),
                           p + "attn.proj.weight": (embed_dim, embed_dim), p + "attn.proj.bias": (embed_dim,),
                           p + "norm1.weight": (embed_dim,), p + "norm1.bias": (embed_dim,), p + "norm2.weight": (embed_dim,), p + "norm2.bias": (embed_dim,),
                           p + "mlp.fc1.weight": (embed_dim * mlp_ratio, embed_dim), p + "mlp.fc1.bias": (embed_dim * mlp_ratio,),
                           p + "mlp.fc2.weight": (embed_dim, embed_dim * mlp_ratio), p + "mlp.fc2.bias": (embed_dim,)})
        return cls(_random_sd(shapes, seed, torch.device(device)), num_heads, merge, device=device)

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "", device="cuda"):
        cfg, sd = _read_dir(path, subfolder)
        cfg = cfg.get("vision_config", cfg)
        sd = {k: v for k, v in sd.items() if "visual." in k or k.startswith(("patch_embed", "blocks", "merger"))}
        return cls(sd, cfg.get("num_heads", 16), cfg.get("spatial_merge_size", 2), cfg.get("hidden_act", "quick_gelu"), device=device)

    @torch.no_grad()
    def __call__(self, hidden_states: torch.Tensor, grid_thw, **_kw):
        """hidden_states: the image processor's flattened patches [S, C*T*p*p]; grid_thw [n_img, 3].
        Returns (last_hidden_state [S, D], pooler_output = merged tokens [S / merge^2, out_dim])."""
        grid = [[int(v) for v in row] for row in (grid_thw.tolist() if torch.is_tensor(grid_thw) else grid_thw)]
        src = hidden_states.to(self.device)
        src = src.contiguous() if src.dtype in (torch.float32, torch.bfloat16) else src.float().contiguous()
        S = src.shape[0]
        assert S == sum(t * h * w for t, h, w in grid)
        if src.dtype == torch.bfloat16 and src.shape[1] == self.patch_w.shape[1] != self.K_in:
            padded = src               # already the GEMM operand (td_qwen2_patchify_u8: device-side preprocessing)
        else:
            assert src.shape[1] == self.K_in
            padded = _hip.cast_pad_rows(src, self.patch_w.shape[1])
        h = _hip.linear(padded, self.patch_w)
        cos, sin = _hip.vision_rope_table(vision_position_ids(grid, self.merge).to(self.device, torch.int32).contiguous(), self.hd, self.theta)
        seg, a0 = [], 0
        for t, gh, gw in grid:                     # full attention inside each frame (cu_seqlens of the reference tower)
            for _ in range(t):
                seg.append((a0, a0 + gh * gw))
                a0 += gh * gw
        # several frames: one packed variable-length launch per layer instead of one launch per frame
        starts = torch.tensor([s0 for s0, _ in seg] + [S], dtype=torch.int32).to(self.device) if len(seg) > 1 else None
        max_len = max(s1 - s0 for s0, s1 in seg)
        for L in self.layers:
            x = _hip.layernorm(h, L["ln1w"], L["ln1b"], 1e-6)
            qkv = _hip.linear(x, L["qkv_w"], L["qkv_b"])
            _hip.rope_half(qkv, 2 * self.H, self.hd, cos, sin)                # q and k heads are adjacent 128-wide slots
            if starts is None:
                a = _hip.attention_padded(qkv, self.H, self.hd ** -0.5)
            else:
                a = _hip.attention_padded_varlen(qkv, self.H, self.hd ** -0.5, starts, max_len)
            h = _hip.linear(a, L["o_w"], L["o_b"], res=h)
            x = _hip.layernorm(h, L["ln2w"], L["ln2b"], 1e-6)
            h = _hip.linear(_hip.linear(x, L["fc1_w"], L["fc1_b"], act=self.act), L["fc2_w"], L["fc2_b"], res=h)
        m = _hip.layernorm(h, self.lnq_w, self.lnq_b, 1e-6).view(S // self.merge ** 2, -1)
        merged = _hip.linear(_hip.linear(m, self.m0_w, self.m0_b, act=_hip.ACT_GELU_ERF), self.m2_w, self.m2_b)
        return _EncoderOutput((h, merged))
