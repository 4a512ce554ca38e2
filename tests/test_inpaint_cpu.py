"""Host logic of FLUX inpainting, without a GPU: the four new torch.ops schemas (registered, no CPU kernel), the new C-ABI entry points
(exported, argument errors before any HIP call), the mask binarization threshold, the host mask helper against PIL, and the
pipeline's refusals (tensor sizes, batch rules, padding_mask_crop, a strength without a step)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
OPS = ("flux_inpaint_step_", "flux_inpaint_mask", "flux_denoise_inpaint_", "flux_denoise_multi_inpaint_")


def test_inpaint_schemas_register_without_cpu_kernel():
    import thinkdiff.ops as ops
    for name in OPS:
        assert name in ops.SCHEMAS
        op = getattr(torch.ops.thinkdiff_hip, name)
        assert str(op.default._schema) == f"thinkdiff_hip::{name}{ops.SCHEMAS[name]}"
    x = torch.zeros(16, 64, dtype=torch.bfloat16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_inpaint_step_(x, x.clone(), x.clone(), None, x.clone(), -0.1, 0.5)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_inpaint_mask(torch.zeros(32, 32, dtype=torch.uint8), 16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_denoise_inpaint_(1, x, [1.0, 0.0], x.clone(), x.clone(), x.clone())
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_denoise_multi_inpaint_([1], [x], [1.0, 0.0], [x.clone()], [x.clone()], [x.clone()], [0])


def test_inpaint_entry_points_exported_and_refuse_bad_arguments():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    for name in ("td_flux_inpaint_step_bf16", "td_flux_inpaint_mask", "td_flux_denoise_inpaint", "td_flux_denoise_multi_inpaint"):
        assert hasattr(lib, name), name
    f32, i64 = ctypes.c_float, ctypes.c_int64
    a, b, c, d = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4))        # never dereferenced: the call must fail first

    def step(x, v, z, nz, m, n):
        return lib.td_flux_inpaint_step_bf16(x, v, z, nz, m, f32(-0.1), f32(0.5), i64(n), None)
    # nulls: x, v, image_latents and mask are required (noise may be NULL)
    for args in [(None, b, c, d, a), (a, None, c, d, b), (a, b, None, d, c), (a, b, c, d, None)]:
        assert step(*args, 64) == 2 and b"null" in lib.td_last_error()
    # a length that is not a multiple of 8
    assert step(a, b, c, None, d, 12) == 2 and b"multiple of 8" in lib.td_last_error()
    assert step(a, b, c, None, d, 0) == 2
    # 16-byte alignment of every operand
    for k in range(5):
        args = [a, b, c, ctypes.c_void_p(5 * 4096), d]
        args[k] = ctypes.c_void_p(args[k].value + 8)
        assert step(*args, 64) == 2 and b"16-byte" in lib.td_last_error()
    # image_latents, noise or mask overlapping x (updated in place)
    assert step(a, b, ctypes.c_void_p(4096 + 64), None, d, 64) == 2 and b"overlap" in lib.td_last_error()
    assert step(a, b, c, ctypes.c_void_p(4096 - 64), d, 64) == 2 and b"overlap" in lib.td_last_error()
    assert step(a, b, c, None, a, 64) == 2 and b"overlap" in lib.td_last_error()

    def mask(src, fmt, H, W, C, out):
        return lib.td_flux_inpaint_mask(src, fmt, H, W, C, out, None)
    assert mask(None, 0, 32, 32, 16, b) == 2 and b"null" in lib.td_last_error()
    assert mask(a, 0, 32, 32, 16, None) == 2 and b"null" in lib.td_last_error()
    for fmt in (2, 7, -1):
        assert mask(a, fmt, 32, 32, 16, b) == 2 and b"format" in lib.td_last_error()
    for H, W in [(24, 32), (32, 40), (0, 32), (8, 8)]:
        assert mask(a, 0, H, W, 16, b) == 2 and b"multiples of 16" in lib.td_last_error()
    assert mask(a, 1, 32, 32, 3, b) == 2 and b"C=3" in lib.td_last_error()
    assert mask(a, 1, 32, 32, 16, ctypes.c_void_p(4096 + 2)) == 2 and b"16-byte" in lib.td_last_error()
    # the engine loops: null arguments come back before any HIP call
    sig = (ctypes.c_float * 2)(1.0, 0.0)
    assert lib.td_flux_denoise_inpaint(None, a, sig, 1, b, c, d, None) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_denoise_inpaint(a, None, sig, 1, b, c, d, None) == 2
    arr = (ctypes.c_void_p * 1)(a.value)
    assert lib.td_flux_denoise_multi_inpaint(arr, arr, 1, sig, 1, None, arr, arr, arr) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_denoise_multi_inpaint(arr, arr, 0, sig, 1, arr, arr, arr, arr) == 2


def test_u8_threshold_is_the_fp32_binarization():
    """mask_processor: pil_to_numpy (float32(u8) / 255), then binarize (>= 0.5); the kernel tests u8 >= 128."""
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(u8 >= 128, (u8.astype(np.float32) / np.float32(255)) >= np.float32(0.5))
    # torch's division gives the same
    t = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(t >= 128, (t.float() / 255) >= 0.5)


def _pil(mode, size, seed):
    from PIL import Image
    g = np.random.default_rng(seed)
    W, H = size
    if mode == "1":
        return Image.fromarray((g.random((H, W)) > 0.5).astype(np.uint8) * 255).convert("1")
    if mode == "L":
        return Image.fromarray(g.integers(0, 256, (H, W), dtype=np.uint8), "L")
    ch = {"RGB": 3, "RGBA": 4}[mode]
    return Image.fromarray(g.integers(0, 256, (H, W, ch), dtype=np.uint8), mode)


@pytest.mark.parametrize("mode", ["1", "L", "RGB", "RGBA"])
@pytest.mark.parametrize("size", [(48, 32), (40, 56), (64, 48)])
def test_host_mask_helper_matches_pil(mode, size):
    """resize (LANCZOS, in the mask's own mode: PIL uses NEAREST for "1") on a size mismatch, then convert("L")"""
    from PIL import Image
    from thinkdiff.models.flux_inpaint import preprocess_mask
    H, W = 48, 64
    im = _pil(mode, size, seed=len(mode) + size[0])
    got = preprocess_mask(im, H, W)
    want = im.resize((W, H), Image.LANCZOS).convert("L") if im.size != (W, H) else im.convert("L")
    assert len(got) == 1 and got[0].dtype == torch.uint8 and tuple(got[0].shape) == (H, W)
    assert np.array_equal(got[0].numpy(), np.array(want))
    # a list gives one mask per entry
    two = preprocess_mask([im, im], H, W)
    assert len(two) == 2 and torch.equal(two[0], two[1])


def test_host_mask_helper_tensor_shapes_and_refusals():
    from thinkdiff.models.flux_inpaint import preprocess_mask
    H, W = 32, 48
    m = torch.rand(H, W, generator=torch.Generator().manual_seed(0))
    for t in (m, m[None], m[None, None]):
        got = preprocess_mask(t, H, W)
        assert len(got) == 1 and got[0].dtype == torch.float32 and torch.equal(got[0], m)
    got = preprocess_mask(torch.stack([m, 1 - m])[:, None], H, W)
    assert len(got) == 2 and torch.equal(got[1], 1 - m)
    for bad in (torch.rand(H, W + 16), torch.rand(1, H + 16, W), torch.rand(2, 1, H, W - 16)):
        with pytest.raises(ValueError, match="not resized"):
            preprocess_mask(bad, H, W)
    for bad in (torch.rand(2, H, W), torch.rand(1, 3, H, W), torch.zeros(H, W, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            preprocess_mask(bad, H, W)
    with pytest.raises(ValueError):
        preprocess_mask([np.zeros((H, W), np.uint8)], H, W)


@pytest.mark.parametrize("B,n_img,n_mask,ok", [(4, 2, 2, True), (4, 1, 2, True), (4, 2, 1, True), (4, 1, 1, True), (4, 4, 2, False),
                                               (4, 2, 4, False), (4, 3, 1, False), (4, 1, 3, False), (6, 2, 3, False), (2, 2, 2, True)])
def test_batch_rules(B, n_img, n_mask, ok):
    from thinkdiff.models.flux_inpaint import check_batches
    if ok:
        check_batches(B, n_img, n_mask)
    else:
        with pytest.raises(ValueError):
            check_batches(B, n_img, n_mask)


def _stub_pipe():
    """No GPU: a transformer stand-in that carries only what the pipeline reads before the first device call."""
    from thinkdiff.models.flux_inpaint import FluxInpaintPipelineRewritePrompt
    tr = SimpleNamespace(device=torch.device("cpu"), dtype=torch.bfloat16, config=SimpleNamespace(in_channels=64, guidance_embeds=True))
    return FluxInpaintPipelineRewritePrompt(transformer=tr)


def test_pipeline_refusals():
    from PIL import Image
    p = _stub_pipe()
    img = Image.new("RGB", (64, 64))
    mask = Image.new("L", (64, 64))
    pe, pool = torch.zeros(2, 8, 32, dtype=torch.bfloat16), torch.zeros(2, 16, dtype=torch.bfloat16)
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pool, height=64, width=64, num_inference_steps=4)
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        p(image=img, mask_image=mask, padding_mask_crop=32, **kw)
    with pytest.raises(NotImplementedError, match="callback_on_step_end"):
        p(image=img, mask_image=mask, callback_on_step_end=lambda *a: {}, **kw)
    with pytest.raises(NotImplementedError, match="sigmas"):
        p(image=img, mask_image=mask, sigmas=[1.0, 0.5], **kw)
    with pytest.raises(NotImplementedError, match="generator"):
        p(image=img, mask_image=mask, generator=[torch.Generator(), torch.Generator()], **kw)
    with pytest.raises(ValueError, match="step"):
        p(image=img, mask_image=mask, strength=0.0, **kw)
    with pytest.raises(ValueError, match="multiples of 16"):
        p(image=img, mask_image=mask, **{**kw, "height": 72})
    with pytest.raises(ValueError, match="mask_image"):
        p(image=img, mask_image=None, **kw)
    with pytest.raises(ValueError, match="not resized"):
        p(image=img, mask_image=torch.rand(1, 1, 32, 64), **kw)
    # 2 prompts x 1 image each = B 2: three images do not divide it; two images and two masks do, with unpacked latents of the wrong shape
    with pytest.raises(ValueError, match="3 images"):
        p(image=[img] * 3, mask_image=mask, **kw)
    with pytest.raises(ValueError, match="3 masks"):
        p(image=img, mask_image=[mask] * 3, **kw)
    with pytest.raises(ValueError, match="unpacked"):
        p(image=[img] * 2, mask_image=[mask] * 2, latents=torch.zeros(2, 16, 64), **kw)
    # 2 prompts x 2 images each = B 4: 4 images and 2 masks do not broadcast against each other
    with pytest.raises(ValueError, match="4 images and 2 masks"):
        p(image=[img] * 4, mask_image=[mask] * 2, num_images_per_prompt=2, **kw)
