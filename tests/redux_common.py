"""FLUX.1 Redux, restated in plain torch for the tests (diffusers is not installed: tests/test_diffusers_probe.py).

* `compose_ref`          the rounding contract of td_redux_compose_bf16 (include/thinkdiff_hip.h): what the kernel is held to, bit for bit.
* `redux_pipeline_ref`   [ext] diffusers FluxPriorReduxPipeline.__call__ after the encoders: batch expansion, the dummy zero embeddings, the
                         concatenation, the per-image scales and the sum over the images.
* `PREPROCESS_DEFAULTS`  the released feature_extractor/preprocessor_config.json; `reference_processor()` is transformers' PIL SigLIP processor on it.
* `tiny_siglip` / `siglip_forward_padded`   a tiny transformers SiglipVisionModel and the plain-torch forward over the padded operands
                         (thinkdiff.models.vision_towers.siglip_padded_weights) -- the tower's graph without a GPU.
"""
import torch
import torch.nn.functional as F

SCALES = [1.0, 0.37, -0.8, 2.5]          # 0.37 is not representable in bf16; one is negative
PREPROCESS_DEFAULTS = dict(do_convert_rgb=True, do_resize=True, size={"height": 384, "width": 384}, resample=3, do_rescale=True,
                           rescale_factor=1 / 255, do_normalize=True, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])      # resample 3 = PIL bicubic
TINY = dict(hidden_size=144, intermediate_size=304, num_hidden_layers=2, num_attention_heads=2, image_size=42, patch_size=14)      # 2 heads of 72, 9 patches


def spread_inputs(shape, seed):
    """bf16 randn whose column magnitudes are spread over 1e-2 .. 1e2."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.logspace(-2, 2, shape[-1])).to(torch.bfloat16)


def compose_ref(text, image, scales, T=0, D=None):
    """text [1 or B, T, D] bf16 or None (T rows of +0.0), image [B, S, D] bf16 or None -> [T + S, D] bf16:
    row r = bf16( sum_b float( bf16( bf16(scales[b]) * x[b, r, :] ) ) ), the sum in fp32 in index order starting from the b = 0 term."""
    s = torch.tensor([float(v) for v in scales], dtype=torch.float32).to(torch.bfloat16)
    B = s.numel()
    ref = image if image is not None else text
    parts = []
    if text is None and T:
        parts.append(torch.zeros(T, ref.shape[-1] if ref is not None else D, dtype=torch.bfloat16))
    for src in (text, image):
        if src is None:
            continue
        src = src.cpu()
        acc = None
        for b in range(B):
            p = (src[b if src.shape[0] > 1 else 0] * s[b]).float()          # a bf16 x bf16 torch op: the product rounded to bf16
            acc = p if acc is None else acc + p
        parts.append(acc.to(torch.bfloat16))
    return torch.cat(parts)


def redux_pipeline_ref(image_embeds, prompt_embeds=None, pooled_prompt_embeds=None, prompt_embeds_scale=1.0, pooled_prompt_embeds_scale=1.0,
                       max_sequence_length=512, pooled_dim=768):
    """FluxPriorReduxPipeline.__call__ from `image_embeds` [B, S, J] on: -> (prompt_embeds [1, T + S, J], pooled_prompt_embeds [1, P]).
        batch_size = number of images;  a float scale -> batch_size * [scale]
        no text: prompt_embeds = zeros(batch_size, max_sequence_length, J), pooled = zeros(batch_size, 768)
        text of batch 1 (one string prompt): repeated for every image
        prompt_embeds = cat([prompt_embeds, image_embeds], dim=1);  *= scale[:, None, None];  pooled *= pooled_scale[:, None]
        prompt_embeds = sum(prompt_embeds, dim=0, keepdim=True);  pooled = sum(pooled, dim=0, keepdim=True)
    The scale-and-sum is taken by `compose_ref` (torch.sum's own order is not part of the contract; on the CPU the two agree)."""
    image_embeds = image_embeds.cpu()
    B, _, J = image_embeds.shape
    scale = [float(prompt_embeds_scale)] * B if isinstance(prompt_embeds_scale, (int, float)) else list(prompt_embeds_scale)
    pscale = [float(pooled_prompt_embeds_scale)] * B if isinstance(pooled_prompt_embeds_scale, (int, float)) else list(pooled_prompt_embeds_scale)
    if prompt_embeds is None:
        prompt_embeds = torch.zeros(B, max_sequence_length, J, dtype=torch.bfloat16)
        pooled_prompt_embeds = torch.zeros(B, pooled_dim, dtype=torch.bfloat16)
    prompt_embeds, pooled_prompt_embeds = prompt_embeds.cpu(), pooled_prompt_embeds.cpu()
    if prompt_embeds.shape[0] == 1:
        prompt_embeds = prompt_embeds.expand(B, -1, -1)
    if pooled_prompt_embeds.shape[0] == 1:
        pooled_prompt_embeds = pooled_prompt_embeds.expand(B, -1)
    stream = torch.cat([prompt_embeds, image_embeds], dim=1)
    return compose_ref(None, stream, scale)[None], compose_ref(None, pooled_prompt_embeds[:, None, :], pscale)


def reference_processor(**overrides):
    from transformers.models.siglip.image_processing_pil_siglip import SiglipImageProcessorPil
    return SiglipImageProcessorPil(**{**PREPROCESS_DEFAULTS, **overrides})


def random_image(h, w, seed):
    import numpy as np
    from PIL import Image
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB")


def tiny_siglip(seed=0, **overrides):
    """transformers SiglipVisionModel (fp32, eval) on bf16-representable weights drawn wide enough for the layers to matter."""
    from transformers import SiglipVisionConfig, SiglipVisionModel
    torch.manual_seed(seed)
    cfg = SiglipVisionConfig(**{**TINY, **overrides})
    with torch.device("meta"):          # every parameter is drawn below: skip transformers' own (slow) initialisation
        ref = SiglipVisionModel(cfg)
    ref = ref.to_empty(device="cpu").eval()
    emb = getattr(ref, "vision_model", ref).embeddings
    emb.position_ids = torch.arange(emb.position_ids.shape[-1])[None]
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "bias" in n:
                p.normal_(0, 0.05)
            elif "norm" in n:
                p.normal_(1.0, 0.1)
            elif "position_embedding" in n:
                p.normal_(0, 0.5)
            elif p.dim() > 1:
                p.normal_(0, 2.0 / p[0].numel() ** 0.5)
            else:
                raise AssertionError(f"parameter {n} is not drawn")
        for p in ref.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return cfg, ref


def vision_sd(ref, prefix=""):
    """The tower's state dict of a SiglipVisionModel under `prefix` ('' or 'vision_model.'), whichever form this transformers uses itself."""
    sd = {k.removeprefix("vision_model."): v.detach().clone() for k, v in ref.state_dict().items()}
    return {prefix + k: v for k, v in sd.items()}


def siglip_hidden_ref(ref, pixel_values, layers=True):
    """last_hidden_state of `ref`; layers=False skips the encoder layers (embeddings -> post_layernorm)."""
    vm = getattr(ref, "vision_model", ref)
    with torch.no_grad():
        if layers:
            return ref(pixel_values=pixel_values).last_hidden_state
        return vm.post_layernorm(vm.embeddings(pixel_values))


def siglip_forward_padded(P, pixel_values, eps=1e-6):
    """The HIP tower's graph in plain torch over the padded operands P = siglip_padded_weights(sd, H): [B, 3, h, w] -> [B, n, D]."""
    D, H, hd, p = P["D"], P["H"], P["hd"], P["patch"]
    pad = lambda x, k: F.pad(x, (0, k - x.shape[-1]))
    outs = []
    for img in pixel_values:
        patches = F.unfold(img[None], kernel_size=p, stride=p)[0].T                      # [n, 3 p p], columns (c, py, px) like Conv2d's weight
        h = pad(patches, P["patch_w"].shape[1]) @ P["patch_w"].T + P["patch_b"] + P["pos"]
        n = h.shape[0]
        for L in P["layers"]:
            x = pad(F.layer_norm(h, (D,), L["ln1w"], L["ln1b"], eps), L["qkv_w"].shape[1])
            q, k, v = (x @ L["qkv_w"].T + L["qkv_b"]).view(n, 3, H, 128).permute(1, 2, 0, 3)          # [H, n, 128] each, columns hd .. 127 zero
            a = torch.softmax(q @ k.transpose(1, 2) * hd ** -0.5, dim=-1) @ v
            h = a.permute(1, 0, 2).reshape(n, H * 128) @ L["o_w"].T + L["o_b"] + h
            x = pad(F.layer_norm(h, (D,), L["ln2w"], L["ln2b"], eps), L["fc1_w"].shape[1])
            h = F.gelu(x @ L["fc1_w"].T + L["fc1_b"], approximate="tanh") @ L["fc2_w"].T + L["fc2_b"] + h
        outs.append(F.layer_norm(h, (D,), P["post_w"], P["post_b"], eps))
    return torch.stack(outs)


def rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
