"""FLUX.1 Kontext without a GPU: the reference / output resolution rules on a table worked by hand, the reference ids, the pipeline's
refusals on a stub transformer (everything refused is refused before the first device call), the new torch.ops schemas, the C ABI's
argument errors (TD_ERR_INVALID before any HIP call), and the CPU restatement against itself.

The three tests under "the restatement against itself" exercise tests/kontext_common.py and eager torch only, no product code: they pass
without the feature and count for nothing as coverage of it.  They are there because the GPU tests lean on that restatement (and on where
eager torch rounds the CFG scale), and a mistake in it should show here, not as a puzzling parity figure on the hardware."""
import ctypes
import inspect
import math
import os
import warnings
from types import SimpleNamespace

import pytest
import torch

from kontext_common import denoise_ref, reference_ids
from oracle import flux_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
OPS = ("flux_set_reference_tokens", "flux_cfg_step_", "flux_denoise_cfg_")


# ---- resolution rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,want", [(1920, 1080, (1392, 752)), (768, 1024, (880, 1184)), (1024, 1024, (1024, 1024)), (4000, 1000, (1568, 672)),
                                      (1000, 4000, (672, 1568))])
def test_reference_resolution_table(w, h, want):
    """(width, height) of the image -> the preferred (width, height) whose aspect ratio is nearest."""
    from thinkdiff.models.flux_kontext import PREFERRED_KONTEXT_RESOLUTIONS, reference_size
    Hr, Wr = reference_size(h, w, True)
    assert (Wr, Hr) == want and want in PREFERRED_KONTEXT_RESOLUTIONS
    # by hand: no other entry is nearer in aspect ratio
    ar = w / h
    assert all(abs(ar - want[0] / want[1]) <= abs(ar - pw / ph) for pw, ph in PREFERRED_KONTEXT_RESOLUTIONS)


def test_preferred_resolutions_are_16_multiples_and_only_one_has_a_64_multiple_mid_block():
    from thinkdiff.models.flux_kontext import PREFERRED_KONTEXT_RESOLUTIONS, reference_size
    assert len(PREFERRED_KONTEXT_RESOLUTIONS) == 17
    assert all(w % 16 == 0 and h % 16 == 0 and w * h <= 1568 * 1568 for w, h in PREFERRED_KONTEXT_RESOLUTIONS)
    assert [(w, h) for w, h in PREFERRED_KONTEXT_RESOLUTIONS if ((w // 8) * (h // 8)) % 64 == 0] == [(1024, 1024)]
    # without _auto_resize: the image's own size, floored to 16
    assert reference_size(100, 170, False) == (96, 160)
    assert reference_size(96, 160, False) == (96, 160)


@pytest.mark.parametrize("h,w,area,want", [(1024, 1024, 1024 ** 2, (1024, 1024)), (1080, 1920, 1024 ** 2, (768, 1360)), (128, 128, 128 ** 2, (128, 128)),
                                           (512, 512, 1024 ** 2, (1024, 1024)), (96, 160, 128 ** 2, (96, 160))])
def test_output_size_rule(h, w, area, want):
    from thinkdiff.models.flux_kontext import output_size
    assert output_size(h, w, area) == want
    ar = w / h
    assert want == (round(math.sqrt(area / ar)) // 16 * 16, round(math.sqrt(area * ar)) // 16 * 16)


def test_reference_ids():
    from thinkdiff.models.flux_kontext import reference_ids as pipe_ids
    ids = pipe_ids(3, 5)
    assert ids.shape == (15, 3) and torch.equal(ids, reference_ids(3, 5))
    assert torch.equal(ids[:, 0], torch.ones(15))
    assert torch.equal(ids[:, 1:], R.latent_image_ids(3, 5)[:, 1:])
    assert ids[7].tolist() == [1.0, 1.0, 2.0]


# ---- refusals on a stub -----------------------------------------------------------------------------------------------------------------
def _stub(in_channels=64, out_channels=None, max_img_tokens=96, encoder_capacity=(128, 128)):
    from thinkdiff.models import FluxKontextPipelineRewritePrompt
    tr = SimpleNamespace(device=torch.device("cpu"), dtype=torch.bfloat16, max_img_tokens=max_img_tokens,
                         config=SimpleNamespace(in_channels=in_channels, out_channels=out_channels, guidance_embeds=True))
    p = FluxKontextPipelineRewritePrompt(transformer=tr)
    p.vae = SimpleNamespace(encoder=SimpleNamespace(max_image_size=encoder_capacity))      # nothing of it may be called
    return p


def _embeds(**over):
    kw = dict(prompt_embeds=torch.zeros(2, 8, 32, dtype=torch.bfloat16), pooled_prompt_embeds=torch.zeros(2, 16, dtype=torch.bfloat16),
              height=64, width=64, max_area=64 * 64, num_inference_steps=4, _auto_resize=False)
    kw.update(over)
    return kw


def test_kontext_pipeline_refusals():
    from PIL import Image
    p = _stub()
    img = Image.new("RGB", (64, 64))
    kw = _embeds()
    for name, val in (("callback_on_step_end", lambda *a: {}), ("sigmas", [1.0, 0.5]), ("joint_attention_kwargs", {"scale": 0.5}),
                      ("ip_adapter_image", img), ("ip_adapter_image_embeds", [torch.zeros(1)]), ("negative_ip_adapter_image", img),
                      ("negative_ip_adapter_image_embeds", [torch.zeros(1)])):
        with pytest.raises(NotImplementedError, match=name):
            p(image=img, **{name: val}, **kw)
    with pytest.raises(NotImplementedError, match="generator"):
        p(image=img, generator=[torch.Generator(), torch.Generator()], **kw)
    with pytest.raises(NotImplementedError, match="several reference images"):
        p(image=[[img, img]], **kw)
    with pytest.raises(ValueError, match="prompt"):
        p(image=img, height=64, width=64, max_area=64 * 64)
    with pytest.raises(ValueError, match="not resized"):
        p(image=torch.rand(1, 3, 40, 64), **kw)
    with pytest.raises(ValueError, match="even height and width"):
        p(image=torch.zeros(1, 16, 5, 8), **kw)
    with pytest.raises(ValueError, match="packed"):
        p(image=img, latents=torch.zeros(2, 16, 8, 8), **kw)
    # 2 prompts x 1 = B 2: 3 reference images do not divide it
    with pytest.raises(ValueError, match="batch size 3"):
        p(image=[img] * 3, **kw)
    # the image stream: 16 latent tokens + 96 reference tokens against a capacity of 96: both numbers and the argument to raise
    big = Image.new("RGB", (128, 192))
    with pytest.raises(ValueError, match=r"16 latent \+ 96 reference tokens = 112 exceeds the transformer's capacity 96.*max_img_tokens"):
        _stub(encoder_capacity=(256, 256))(image=big, **kw)
    # the encoder's capacity, with the size that serves every preferred resolution
    with pytest.raises(ValueError, match=r"192 x 128 = 24576 pixels exceeds the VAE encoder's capacity 128 x 128.*1568, 1568"):
        _stub(max_img_tokens=4096)(image=Image.new("RGB", (192, 128)), **kw)
    # _auto_resize sends a small picture to a preferred size: the refusal names that size, so the rule ran on the host first
    with pytest.raises(ValueError, match="1024 x 1024"):
        p(image=img, **{**kw, "_auto_resize": True})
    # true_cfg_scale > 1 without a negative prompt: a warning and the plain loop (which then fails on the stub's missing device, later)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(Exception):
            p(image=None, true_cfg_scale=4.0, **kw)
    assert any("classifier-free guidance is not enabled" in str(x.message) for x in w)
    # a negative prompt with true_cfg_scale <= 1 is ignored, with a warning
    neg = dict(negative_prompt_embeds=torch.zeros(2, 8, 32, dtype=torch.bfloat16), negative_pooled_prompt_embeds=torch.zeros(2, 16, dtype=torch.bfloat16))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(Exception):
            p(image=None, **neg, **kw)
    assert any("negative_prompt is passed but classifier-free guidance is not enabled" in str(x.message) for x in w)
    # a keyword the call does not have is an error, not the plain loop
    with pytest.raises(TypeError, match="negative_promt"):
        p(image=img, negative_promt="x", **kw)
    for name in ("callback_on_step_end", "sigmas", "ip_adapter_image"):      # None of a refused keyword is accepted as "not set"
        with pytest.raises(ValueError, match="batch size 3"):
            p(image=[img] * 3, **{name: None}, **kw)
    # the output size rule warns when it changes what the caller asked for
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(ValueError, match=r"12 latent \+ 96 reference"):
            _stub(encoder_capacity=(256, 256))(image=big, **{**kw, "height": 70, "width": 64})
    assert any("adjusted to 64 and 48" in str(x.message) for x in w)


@pytest.mark.parametrize("cin,cout", [(384, 64), (128, 64), (128, 128), (64, 32)])
def test_kontext_pipeline_names_both_channel_counts(cin, cout):
    from PIL import Image
    p = _stub(cin, cout)
    with pytest.raises(ValueError, match=f"in_channels = {cin}, out_channels = {cout}"):
        p(image=Image.new("RGB", (64, 64)), **_embeds())


def test_call_surface():
    from thinkdiff.models import FluxKontextPipelineRewritePrompt
    sig = inspect.signature(FluxKontextPipelineRewritePrompt.__call__).parameters
    want = {"image": None, "prompt": None, "prompt_2": None, "negative_prompt": None, "negative_prompt_2": None, "true_cfg_scale": 1.0,
            "height": None, "width": None, "num_inference_steps": 28, "guidance_scale": 3.5, "num_images_per_prompt": 1, "generator": None,
            "latents": None, "prompt_embeds": None, "pooled_prompt_embeds": None, "negative_prompt_embeds": None,
            "negative_pooled_prompt_embeds": None, "output_type": "pil", "return_dict": True, "max_sequence_length": 512,
            "max_area": 1024 ** 2, "_auto_resize": True}
    for k, v in want.items():
        assert k in sig and sig[k].default == v, k


# ---- op layer and C ABI ----------------------------------------------------------------------------------------------------------------
def test_kontext_schemas_register_without_cpu_kernel():
    import thinkdiff.ops as ops
    for name in OPS:
        assert name in ops.SCHEMAS
        op = getattr(torch.ops.thinkdiff_hip, name)
        assert str(op.default._schema) == f"thinkdiff_hip::{name}{ops.SCHEMAS[name]}"
    x = torch.zeros(16, 64, dtype=torch.bfloat16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_cfg_step_(x, x.clone(), x.clone(), 3.5, -0.1)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_set_reference_tokens(1, x, torch.zeros(16, 3))
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.flux_denoise_cfg_(1, 2, x, [1.0, 0.0], 3.5)


def test_kontext_entry_points_exported_and_refuse_bad_arguments():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    for name in ("td_flux_set_reference_tokens", "td_flux_reference_tokens", "td_flux_cfg_step_bf16", "td_flux_denoise_cfg",
                 "td_softmax_rows_strided_f32_bf16"):
        assert hasattr(lib, name), name
    f32, i64 = ctypes.c_float, ctypes.c_int64
    a, b, c = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3))        # never dereferenced: the call must fail first

    def step(x, vp, vn, n):
        return lib.td_flux_cfg_step_bf16(x, vp, vn, f32(3.5), f32(-0.1), i64(n), None)
    for args in [(None, b, c), (a, None, c), (a, b, None)]:
        assert step(*args, 64) == 2 and b"null" in lib.td_last_error()
    assert step(a, b, c, 12) == 2 and b"multiple of 8" in lib.td_last_error()
    assert step(a, b, c, 0) == 2
    for k in range(3):
        args = [a, b, c]
        args[k] = ctypes.c_void_p(args[k].value + 8)
        assert step(*args, 64) == 2 and b"16-byte" in lib.td_last_error()
    assert step(a, ctypes.c_void_p(4096 + 64), c, 64) == 2 and b"overlap" in lib.td_last_error()
    assert step(a, b, ctypes.c_void_p(4096 - 64), 64) == 2 and b"overlap" in lib.td_last_error()
    assert step(a, b, a, 64) == 2 and b"overlap" in lib.td_last_error()
    # the engine entry points: null arguments come back before any HIP call
    assert lib.td_flux_set_reference_tokens(None, a, 16, b, None) == 2 and b"null" in lib.td_last_error()
    n = ctypes.c_int(7)
    assert lib.td_flux_reference_tokens(None, ctypes.byref(n)) == 2 and b"null" in lib.td_last_error()
    sig = (ctypes.c_float * 2)(1.0, 0.0)
    assert lib.td_flux_denoise_cfg(None, a, b, sig, 1, f32(3.5), None) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_denoise_cfg(a, None, b, sig, 1, f32(3.5), None) == 2
    assert lib.td_flux_denoise_cfg(a, b, None, sig, 1, f32(3.5), None) == 2
    assert lib.td_flux_denoise_cfg(a, b, c, None, 1, f32(3.5), None) == 2
    assert lib.td_flux_denoise_cfg(a, a, c, sig, 1, f32(3.5), None) == 2 and b"same" in lib.td_last_error()
    # the strided softmax: stride below the column count, odd strides, nulls
    sm = lambda s, p, rows, cols, ld: lib.td_softmax_rows_strided_f32_bf16(s, p, rows, cols, ld, f32(1.0), None)
    assert sm(None, b, 4, 64, 64) == 2 and b"null" in lib.td_last_error()
    assert sm(a, b, 4, 64, 60) == 2 and b"stride" in lib.td_last_error()
    assert sm(a, b, 4, 64, 66) == 2 and b"stride" in lib.td_last_error()
    assert sm(a, b, 4, 62, 64) == 2 and b"multiple of 4" in lib.td_last_error()


# ---- the restatement against itself ----------------------------------------------------------------------------------------------------
def _case(seed=4):
    cfg = R.tiny_config(num_layers=1, num_single_layers=1)
    sd = R.init_weights(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed)
    h2 = w2 = 4
    lat = torch.randn(1, h2 * w2, 64, generator=g).bfloat16()
    ref = torch.randn(1, 8, 64, generator=g).bfloat16()
    pe = torch.randn(1, 8, cfg.joint_attention_dim, generator=g).bfloat16()
    pool = torch.randn(1, cfg.pooled_projection_dim, generator=g).bfloat16()
    return cfg, sd, h2, w2, lat, ref, pe, pool


def test_restatement_without_reference_is_the_oracle_loop():
    cfg, sd, h2, w2, lat, ref, pe, pool = _case()
    want = R.denoise(sd, cfg, lat, pe, pool, h2, w2, 2, guidance_scale=3.5)
    assert torch.equal(denoise_ref(sd, cfg, lat, None, None, pe, pool, h2, w2, 2), want)
    assert torch.equal(denoise_ref(sd, cfg, lat, ref[:, :0], reference_ids(2, 4)[:0], pe, pool, h2, w2, 2), want)
    with_ref = denoise_ref(sd, cfg, lat, ref, reference_ids(2, 4), pe, pool, h2, w2, 2)
    assert with_ref.shape == want.shape and not torch.equal(with_ref, want)


def test_restatement_cfg_with_equal_branches_is_the_plain_loop():
    """pos == neg: d = 0 exactly, so v = neg + scale * 0 = neg whatever the scale."""
    cfg, sd, h2, w2, lat, ref, pe, pool = _case(5)
    rid = reference_ids(2, 4)
    plain = denoise_ref(sd, cfg, lat, ref, rid, pe, pool, h2, w2, 2)
    for scale in (1.0, 3.5, 7.25):
        assert torch.equal(denoise_ref(sd, cfg, lat, ref, rid, pe, pool, h2, w2, 2, neg=(pe, pool), scale=scale), plain)
    g = torch.Generator().manual_seed(1)
    neg = (torch.randn(1, 6, cfg.joint_attention_dim, generator=g).bfloat16(), torch.randn(1, cfg.pooled_projection_dim, generator=g).bfloat16())
    assert not torch.equal(denoise_ref(sd, cfg, lat, ref, rid, pe, pool, h2, w2, 2, neg=neg, scale=3.5), plain)


def test_eager_cpu_torch_keeps_the_cfg_scale_in_fp32():
    """`s * d` with a Python float s on a bf16 tensor: bf16(float(d) * fp32(s)), not bf16(float(d) * float(bf16(s))) -- the rounding
    point td_flux_cfg_step_kernel restates (the GPU test holds the kernel to the device's eager statements)."""
    d = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    d = d[torch.isfinite(d.float())]
    s = 3.7
    got = s * d
    f32 = (d.float() * torch.tensor(s, dtype=torch.float32)).bfloat16()
    b16 = (d.float() * torch.tensor(s).bfloat16().float()).bfloat16()
    assert torch.equal(got.view(torch.int16), f32.view(torch.int16))
    assert int((f32.view(torch.int16) != b16.view(torch.int16)).sum()) > 1000
