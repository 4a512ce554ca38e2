"""FLUX.1 Redux without a GPU: the C entry's refusals, the compose restatement against torch's own sum, the default preprocessing against
transformers' PIL SigLIP processor, the padded-weight construction against transformers' SiglipVisionModel, the pipeline's refusals (stub encoders:
nothing may reach the GPU) and the checkpoint directory reader."""
import ctypes
import json
import os

import pytest
import torch

import redux_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
i64 = ctypes.c_int64


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    return lib


def test_library_exports_the_entry_and_abi_8(L):
    assert hasattr(L, "td_redux_compose_bf16") and L.td_abi_version() >= 8
    import thinkdiff.ops as ops
    assert "redux_compose" in ops.SCHEMAS
    assert str(torch.ops.thinkdiff_hip.redux_compose.default._schema) == "thinkdiff_hip::redux_compose" + ops.SCHEMAS["redux_compose"]
    from thinkdiff import _hip
    assert callable(_hip.redux_compose) and hasattr(_hip.lib(), "td_redux_compose_bf16")


def test_entry_refuses_bad_arguments_without_a_gpu(L):
    one = ctypes.c_void_p(256)                     # 16-byte aligned, never dereferenced: every call must fail before any HIP call
    sc = (ctypes.c_float * 16)(*([1.0] * 16))

    def call(text=one, tbs=4096 * 8, T=8, image=one, ibs=4096 * 8, S=8, scales=sc, B=2, D=4096, out=one, ldo=4096):
        rc = L.td_redux_compose_bf16(text, i64(tbs), T, image, i64(ibs), S, scales, B, D, out, i64(ldo), None)
        return rc, L.td_last_error()

    cases = {
        "D % 8": (dict(D=4100, ldo=4104), b"D="),
        "B = 0": (dict(B=0), b"B="),
        "B = 17": (dict(B=17), b"B="),
        "T < 0": (dict(T=-1), b"T="),
        "S < 0": (dict(S=-1), b"S="),
        "T + S == 0": (dict(T=0, S=0), b"T="),
        "ldo < D": (dict(ldo=4088), b"ldo="),
        "image NULL with S > 0": (dict(image=None), b"image"),
        "scales NULL": (dict(scales=None), b"scales"),
        "rows x D past INT32_MAX": (dict(T=2 ** 19, S=1), b"32-bit index"),
        "T alone past INT32_MAX / D": (dict(T=2 ** 31 - 1, S=2 ** 31 - 1), b"32-bit index"),
    }
    for what, (kw, needle) in cases.items():
        rc, msg = call(**kw)
        assert rc == 2, (what, rc, msg)
        assert needle in msg and b"td_redux_compose" in msg, (what, msg)
    # S = 0 without an image and T = 0 without a text are argument forms, not errors: the refusal that follows is the next one in line
    rc, msg = call(image=None, S=0, scales=None)
    assert rc == 2 and b"scales" in msg
    rc, msg = call(text=None, T=0, scales=None)
    assert rc == 2 and b"scales" in msg


def test_patchify_refuses_an_image_smaller_than_the_patch(L):
    """384 = 27 x 14 + 6: the patch operand drops the trailing pixels as Conv2d(kernel = stride = 14) does (checked on the GPU at the released
    widths); what stays refused is an image with no whole patch, and a Kpad below 3 p p."""
    one = ctypes.c_void_p(256)
    assert L.td_patchify_bf16(one, 1, 3, 13, 384, 14, one, 640, None) == 2 and b"smaller than the patch" in L.td_last_error()
    assert L.td_patchify_bf16(one, 1, 3, 384, 384, 14, one, 576, None) == 2 and b"Kpad" in L.td_last_error()


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_compose_restatement_equals_torch_sum(B):
    x = C.spread_inputs((B, 37, 4096), seed=1)
    s = torch.tensor(C.SCALES[:B], dtype=torch.bfloat16)
    want = (x * s[:, None, None]).sum(0)
    got = C.compose_ref(None, x, C.SCALES[:B])
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    both = C.compose_ref(x[:, :5], x[:, 5:], C.SCALES[:B])          # the [text | image] split changes nothing
    assert torch.equal(both, want)


def test_default_preprocessing_equals_the_pil_siglip_processor():
    from thinkdiff.models.flux_redux import ReduxDefaultImageProcessor
    img = C.random_image(200, 300, seed=0)
    want = C.reference_processor().preprocess(images=[img], return_tensors="pt").pixel_values
    got = ReduxDefaultImageProcessor().preprocess(images=[img]).pixel_values
    assert got.shape == (1, 3, 384, 384) and got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(ReduxDefaultImageProcessor()(img).pixel_values, want)


@pytest.mark.parametrize("prefix", ["", "vision_model."])
def test_padded_weights_equal_transformers_siglip(prefix):
    from thinkdiff.models.vision_towers import siglip_padded_weights
    cfg, ref = C.tiny_siglip(seed=0)
    pix = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(1))
    want = C.siglip_hidden_ref(ref, pix)
    assert C.rel_rmse(C.siglip_hidden_ref(ref, pix, layers=False), want) > 0.3          # the layers matter in this draw
    sd = C.vision_sd(ref, prefix)
    assert any(k.startswith(prefix + "head.") for k in sd)                                # the pooling head is present and ignored
    P = siglip_padded_weights(sd, cfg.num_attention_heads)
    L0 = P["layers"][0]
    assert P["patch_w"].shape == (144, 640) and L0["qkv_w"].shape == (3 * 2 * 128, 192) and L0["o_w"].shape == (144, 256)
    assert L0["fc1_w"].shape == (320, 192) and L0["fc1_b"].shape == (320,) and L0["fc2_w"].shape == (144, 320) and len(P["layers"]) == 2
    assert not L0["fc1_w"][304:].any() and not L0["fc1_b"][304:].any() and not L0["fc2_w"][:, 304:].any() and not L0["qkv_w"][:, 144:].any()
    got = C.siglip_forward_padded(P, pix, cfg.layer_norm_eps)
    e = C.rel_rmse(got, want)
    print(f"padded weights vs SiglipVisionModel, fp32: rel-RMSE {e:.2e}")
    assert got.shape == (2, 9, 144) and e < 1e-5


def test_released_mlp_width_pads_to_4352():
    from thinkdiff.models.vision_towers import siglip_padded_weights
    z = lambda *s: torch.zeros(*s)
    sd = {"embeddings.patch_embedding.weight": z(64, 3, 14, 14), "embeddings.patch_embedding.bias": z(64), "embeddings.position_embedding.weight": z(4, 64),
          "post_layernorm.weight": z(64), "post_layernorm.bias": z(64)}
    p = "encoder.layers.0."
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        sd.update({p + f"self_attn.{n}.weight": z(64, 64), p + f"self_attn.{n}.bias": z(64)})
    sd.update({p + "layer_norm1.weight": z(64), p + "layer_norm1.bias": z(64), p + "layer_norm2.weight": z(64), p + "layer_norm2.bias": z(64),
               p + "mlp.fc1.weight": z(4304, 64), p + "mlp.fc1.bias": z(4304), p + "mlp.fc2.weight": z(64, 4304), p + "mlp.fc2.bias": z(64)})
    P = siglip_padded_weights(sd, 1)
    assert P["layers"][0]["fc1_w"].shape == (4352, 64) and P["layers"][0]["fc2_w"].shape == (64, 4352) and P["patch_w"].shape == (64, 640)


class _Stub:
    """An encoder that must not be reached."""
    txt_in_features = 64
    device = torch.device("cpu")

    def __call__(self, *a, **k):
        raise AssertionError("a refusal must come before any encoder (GPU) work")

    preprocess = __call__


def _stub_pipe(**kw):
    from thinkdiff.models import FluxPriorReduxPipelineRewritePrompt
    return FluxPriorReduxPipelineRewritePrompt(_Stub(), _Stub(), _Stub(), **kw)


def test_pipeline_refusals_name_what_was_asked():
    pipe = _stub_pipe()
    pix = torch.zeros(2, 3, 42, 42)
    pe, pool = torch.zeros(2, 8, 64, dtype=torch.bfloat16), torch.zeros(2, 32, dtype=torch.bfloat16)
    cases = [
        (dict(image=pix, prompt="a cat"), "prompt"),
        (dict(image=pix, prompt_embeds=pe), "pooled_prompt_embeds"),
        (dict(image=pix, pooled_prompt_embeds=pool), "prompt_embeds"),
        (dict(image=pix, prompt_embeds=torch.zeros(3, 8, 64, dtype=torch.bfloat16), pooled_prompt_embeds=pool), "prompt_embeds has batch 3"),
        (dict(image=pix, prompt_embeds=pe, pooled_prompt_embeds=torch.zeros(3, 32, dtype=torch.bfloat16)), "pooled_prompt_embeds has batch 3"),
        (dict(image=pix, prompt_embeds_scale=[1.0, 0.5, 0.25]), "prompt_embeds_scale"),
        (dict(image=pix, pooled_prompt_embeds_scale=[1.0]), "pooled_prompt_embeds_scale"),
        (dict(image=torch.zeros(17, 3, 42, 42)), "17 images"),
        (dict(image=[object()] * 17), "17 images"),
        (dict(image=pix, prompt_embeds=torch.zeros(2, 8, 72, dtype=torch.bfloat16), pooled_prompt_embeds=pool), "width 72"),
    ]
    for kw, needle in cases:
        with pytest.raises(ValueError) as ei:
            pipe(**kw)
        assert needle in str(ei.value), (kw.keys(), str(ei.value))
    with pytest.raises(AssertionError):          # a well-formed call does go on to the encoders
        pipe(image=pix, prompt_embeds=pe, pooled_prompt_embeds=pool)


def _write_dir(root, with_preprocessor=True):
    from safetensors.torch import save_file
    cfg, ref = C.tiny_siglip(seed=2)
    for sub in ("image_encoder", "image_embedder"):
        (root / sub).mkdir()
    save_file({k: v.contiguous() for k, v in C.vision_sd(ref, "vision_model.").items()}, str(root / "image_encoder" / "model.safetensors"))
    (root / "image_encoder" / "config.json").write_text(json.dumps({"model_type": "siglip_vision_model", **C.TINY, "layer_norm_eps": 1e-6,
                                                                       "hidden_act": "gelu_pytorch_tanh"}))
    save_file({"redux_up.weight": torch.zeros(192, 144), "redux_up.bias": torch.zeros(192), "redux_down.weight": torch.zeros(64, 192),
               "redux_down.bias": torch.zeros(64)}, str(root / "image_embedder" / "diffusion_pytorch_model.safetensors"))
    (root / "image_embedder" / "config.json").write_text(json.dumps({"_class_name": "ReduxImageEncoder", "redux_dim": 144, "txt_in_features": 64}))
    if with_preprocessor:
        (root / "feature_extractor").mkdir()
        (root / "feature_extractor" / "preprocessor_config.json").write_text(json.dumps({"image_processor_type": "SiglipImageProcessor", **C.PREPROCESS_DEFAULTS}))


def test_from_pretrained_finds_its_parts(tmp_path):
    from thinkdiff.models import FluxPriorReduxPipelineRewritePrompt as Pipe
    from thinkdiff.models.flux_redux import ReduxDefaultImageProcessor
    with pytest.raises(FileNotFoundError):
        Pipe.from_pretrained("black-forest-labs/FLUX.1-Redux-dev")
    with pytest.raises(FileNotFoundError):
        Pipe.from_pretrained(str(tmp_path / "absent"))
    a = tmp_path / "a"
    a.mkdir()
    _write_dir(a)
    parts = Pipe.read_parts(str(a))
    cfg, sd = parts["image_encoder"]
    assert cfg["num_attention_heads"] == 2 and "vision_model.encoder.layers.1.mlp.fc2.weight" in sd
    assert parts["image_embedder"][1]["redux_up.weight"].shape == (192, 144) and parts["image_embedder"][0]["txt_in_features"] == 64
    assert not parts["text_encoder"] and not parts["text_encoder_2"]
    img = C.random_image(50, 70, seed=3)
    want = C.reference_processor().preprocess(images=[img], return_tensors="pt").pixel_values
    assert type(parts["feature_extractor"]).__name__.startswith("SiglipImageProcessor")
    assert torch.equal(parts["feature_extractor"].preprocess(images=[img], return_tensors="pt").pixel_values, want)
    b = tmp_path / "b"
    b.mkdir()
    _write_dir(b, with_preprocessor=False)
    parts = Pipe.read_parts(str(b))
    assert isinstance(parts["feature_extractor"], ReduxDefaultImageProcessor)
    assert torch.equal(parts["feature_extractor"].preprocess(images=[img]).pixel_values, want)
    (b / "image_embedder" / "diffusion_pytorch_model.safetensors").unlink()
    with pytest.raises(FileNotFoundError):
        Pipe.read_parts(str(b))
