"""FLUX ControlNet without a GPU: identities of the test-local reference (tests/controlnet_common.py), the block-index rule and the
`controlnet_keep` schedule against hand-written tables, the sensitivity the GPU tests rely on, the C ABI's argument errors
(TD_ERR_INVALID before any HIP call) and the refusals of the loader and the pipeline (refused before the first device call)."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import controlnet_common as C
from oracle import flux_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
BF = torch.bfloat16


def _call_args(cfg, lat, pe, pool, dtype):
    t = (torch.tensor([0.61]).bfloat16() if dtype == BF else torch.tensor([0.61]).bfloat16().float())
    ids, tids = R.latent_image_ids(C.H2, C.W2).to(dtype), torch.zeros(pe.shape[0], 3).to(dtype)
    return lat[None].to(dtype), pe[None].to(dtype), pool[None].to(dtype), t, ids, tids, torch.tensor([3.5])


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ---- reference identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", list(C.CASES))
def test_zero_output_linears_and_scale_zero_reproduce_the_plain_transformer(case, dtype):
    """All-zero output Linears (the published `zero_module` init) and conditioning scale 0 both give R.transformer_forward exactly."""
    n_d, n_s, num_mode, mode = C.CASES[case]
    cfg, cfg_cn = C.main_config(), C.cn_config(n_d, n_s)
    sd = _cast(R.init_weights(cfg, seed=C.SEED_MAIN), dtype)
    sd_cn = _cast(C.cn_init_weights(cfg_cn, num_mode, seed=C.SEED_CN), dtype)
    lat, cond, _, pe, pool = C.inputs(cfg, C.H2 * C.W2, C.T_TXT, C.SEED_IN)
    x, e, p, t, ids, tids, g = _call_args(cfg, lat, pe, pool, dtype)
    plain = R.transformer_forward(sd, cfg, x, e, p, t, ids, tids, g)
    zero = C.controlled_forward_ref(sd, cfg, C.zero_outputs(sd_cn), cfg_cn, x, cond[None].to(dtype), mode, e, p, t, ids, tids, g, 1.0)
    assert torch.equal(zero, plain)
    bs, ss = C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond[None].to(dtype), mode, e, p, t, ids, tids, None, 0.0)
    assert len(bs) == n_d and len(ss) == n_s and all(float(s.abs().max()) == 0.0 for s in bs + ss)
    assert torch.equal(C.transformer_forward_ref(sd, cfg, x, e, p, t, ids, tids, g, bs, ss), plain)
    assert torch.equal(C.controlled_forward_ref(sd, cfg, sd_cn, cfg_cn, x, cond[None].to(dtype), mode, e, p, t, ids, tids, g, 0.0), plain)
    assert torch.equal(C.transformer_forward_ref(sd, cfg, x, e, p, t, ids, tids, g), plain)


def test_union_reference_needs_a_mode_and_lengthens_the_text_stream():
    cfg_cn = C.cn_config(2, 3)
    sd_cn = C.cn_init_weights(cfg_cn, 2, seed=C.SEED_CN)
    lat, cond, _, pe, pool = C.inputs(cfg_cn, C.H2 * C.W2, C.T_TXT, C.SEED_IN)
    x, e, p, t, ids, tids, g = _call_args(cfg_cn, lat, pe, pool, BF)
    with pytest.raises(ValueError, match="controlnet_mode"):
        C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond[None], None, e, p, t, ids, tids, None)
    a, _ = C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond[None], 0, e, p, t, ids, tids, None)
    b, _ = C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond[None], 1, e, p, t, ids, tids, None)
    assert a[0].shape == (1, C.H2 * C.W2, cfg_cn.inner_dim) and not torch.equal(a[0], b[0])


def test_python_float_scale_is_an_fp32_operand_of_the_bf16_multiply():
    """`sample * conditioning_scale` in eager torch: the product of the fp32 values rounds once (the scale is not rounded to bf16 first)."""
    r = torch.randn(4096, generator=torch.Generator().manual_seed(1)).bfloat16()
    for s in (0.7, 0.35, 1.0):
        assert torch.equal(r * s, (r.float() * s).bfloat16())
    assert not torch.equal(r * 0.7, r * torch.tensor(0.7).bfloat16())


# ---- the index rule and the keep schedule -------------------------------------------------------------------------------------------------
INDEX_TABLES = {
    (19, 5): [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4],
    (38, 10): [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8, 9, 9],
    (2, 1): [0, 0],
    (3, 2): [0, 0, 1],
    (4, 3): [0, 0, 1, 1],      # ceil(4 / 3) = 2: sample 2 is never reached
    (19, 4): [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3],
}


@pytest.mark.parametrize("L,n", list(INDEX_TABLES))
def test_block_index_rule(L, n):
    from thinkdiff.models.flux_controlnet import sample_index
    want = INDEX_TABLES[(L, n)]
    assert [C.sample_index(i, L, n) for i in range(L)] == want
    assert [sample_index(i, L, n) for i in range(L)] == want
    assert max(want) < n
    if (L, n) == (4, 3):
        assert 2 not in want


@pytest.mark.parametrize("start,end,want", [(0.0, 1.0, [1, 1, 1, 1]), (0.0, 0.5, [1, 1, 0, 0]), (0.25, 0.75, [0, 1, 1, 0]), (0.0, 0.0, [0, 0, 0, 0])])
def test_keep_schedule(start, end, want):
    from thinkdiff.models.flux_controlnet import controlnet_keep
    assert C.keep_schedule(4, start, end) == [float(v) for v in want]
    assert controlnet_keep(4, start, end) == [float(v) for v in want]
    assert controlnet_keep(28, 0.0, 0.5) == [1.0] * 14 + [0.0] * 14


# ---- sensitivity of the reference, with the seeds the GPU tests use --------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.CASES))
def test_reference_is_sensitive_to_the_residuals_and_to_the_control_image(case):
    n_d, n_s, num_mode, mode = C.CASES[case]
    cfg, cfg_cn = C.main_config(), C.cn_config(n_d, n_s)
    sd, sd_cn = R.init_weights(cfg, seed=C.SEED_MAIN), C.cn_init_weights(cfg_cn, num_mode, seed=C.SEED_CN)
    lat, cond, cond2, pe, pool = C.inputs(cfg, C.H2 * C.W2, C.T_TXT, C.SEED_IN)
    x, e, p, t, ids, tids, g = _call_args(cfg, lat, pe, pool, BF)
    plain = R.transformer_forward(sd, cfg, x, e, p, t, ids, tids, g)
    this = C.controlled_forward_ref(sd, cfg, sd_cn, cfg_cn, x, cond[None], mode, e, p, t, ids, tids, g, C.SCALE)
    other = C.controlled_forward_ref(sd, cfg, sd_cn, cfg_cn, x, cond2[None], mode, e, p, t, ids, tids, g, C.SCALE)
    d_plain, d_other = C.rel_rmse(plain, this), C.rel_rmse(other, this)
    sa, _ = C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond[None], mode, e, p, t, ids, tids, None)
    sb, _ = C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond2[None], mode, e, p, t, ids, tids, None)
    d_samples = C.rel_rmse(torch.cat(sb), torch.cat(sa))
    print(f"{case}: residuals move the output by {d_plain:.3f}, another control image by {d_other:.3f}, the samples by {d_samples:.3f}")
    assert d_other > 0.1 and d_plain > 0.1 and d_samples > 0.1


# ---- the C ABI refuses bad arguments before any HIP call ------------------------------------------------------------------------------------
def _lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    lib.td_flux_residual_inject_bf16.argtypes = [vp, i64, vp, i64, i32, i32, f32, vp]
    return lib


def test_abi_version_names_the_controlnet():
    assert _lib().td_abi_version() >= 4


def test_inject_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    h, r = 1 << 20, 1 << 22      # never dereferenced: every check precedes the launch
    inj = lambda **k: lib.td_flux_residual_inject_bf16(k.get("h", h), k.get("ldh", 64), k.get("r", r), k.get("ldr", 64), k.get("rows", 4), k.get("D", 64), 0.7, None)
    assert inj(h=None) == 2 and b"null" in lib.td_last_error()
    assert inj(r=None) == 2 and b"null" in lib.td_last_error()
    assert inj(h=h + 8) == 2 and b"16-byte" in lib.td_last_error()
    assert inj(r=r + 2) == 2 and b"16-byte" in lib.td_last_error()
    assert inj(D=60, ldh=64, ldr=64) == 2 and b"multiple of 8" in lib.td_last_error()
    assert inj(ldh=68) == 2 and b"multiples of 8" in lib.td_last_error()
    assert inj(ldr=56) == 2 and b"at least D" in lib.td_last_error()
    assert inj(rows=0) == 2
    # overlap: r inside h's extent, r == h, and r just behind h's last row (allowed to touch, not to overlap)
    assert inj(r=h + 64) == 2 and b"overlap" in lib.td_last_error()
    assert inj(r=h) == 2 and b"overlap" in lib.td_last_error()
    assert inj(h=r + 16, ldh=128) == 2 and b"overlap" in lib.td_last_error()
    assert inj(ldh=1 << 40) == 2 and b"32-bit" in lib.td_last_error()


def test_controlnet_entry_points_refuse_null_arguments_without_a_gpu():
    lib = _lib()
    one = ctypes.c_void_p(256)
    assert lib.td_flux_controlnet_create(None, 0, 64, 64, 4, None) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_controlnet_set_mode(None, 0) == 2
    assert lib.td_flux_controlnet_set_condition(None, one, None) == 2
    assert lib.td_flux_controlnet_forward(None, one, 0, None) == 2
    assert lib.td_flux_controlnet_samples(None, None, None, None, None, None, None) == 2
    assert lib.td_flux_controlnet_read_sample(None, 0, one, None) == 2
    assert lib.td_flux_attach_controlnet(None, None) == 2
    assert lib.td_flux_set_controlnet_scales(None, None, 0) == 2


def test_controlnet_create_refuses_bad_configurations_without_a_gpu():
    from thinkdiff import _hip
    lib = _lib()
    lib.td_flux_controlnet_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    def create(in_channels=64, n_d=1, n_s=0, out_channels=0, num_mode=0):
        cfg = _hip.TdFluxConfig(in_channels, n_d, n_s, 4, 128, 512, 256, 0, 4, (ctypes.c_int * 3)(16, 56, 56), 10000.0, out_channels)
        h = ctypes.c_void_p()
        rc = lib.td_flux_controlnet_create(ctypes.byref(cfg), num_mode, 64, 64, 4, ctypes.byref(h))
        return rc, lib.td_last_error(), h

    rc, msg, h = create(n_d=0)
    assert rc == 2 and b"num_layers=0" in msg and not h.value
    rc, msg, h = create(in_channels=128, out_channels=64)
    assert rc == 2 and b"in_channels=128, out_channels=64" in msg and not h.value
    rc, msg, h = create(num_mode=-1)
    assert rc == 2 and b"num_mode=-1" in msg and not h.value
    # the struct itself is the transformer's: a ControlNet's kind and num_mode travel as arguments
    assert [n for n, _ in _hip.TdFluxConfig._fields_][-1] == "out_channels"


# ---- loader and pipeline refusals on the host -----------------------------------------------------------------------------------------------
def test_config_keys_and_loader_refusals():
    from thinkdiff.models import FluxControlNetConfig, FluxControlNetModel
    j = FluxControlNetModel.config_from_json
    c = j({"_class_name": "FluxControlNetModel", "num_layers": 5, "num_single_layers": 10, "num_mode": 10, "guidance_embeds": False,
           "attention_head_dim": 128, "num_attention_heads": 24, "in_channels": 64, "conditioning_embedding_channels": None, "extra": 1})
    assert isinstance(c, FluxControlNetConfig) and (c.num_layers, c.num_single_layers, c.num_mode, c.guidance_embeds) == (5, 10, 10, False)
    assert c.inner_dim == 3072 and c.to_hip().guidance_embeds == 0 and c.to_hip().num_single_layers == 10
    assert j({"num_layers": 2, "num_single_layers": 0}).num_mode is None
    with pytest.raises(NotImplementedError, match="conditioning_embedding_channels=16"):
        j({"num_layers": 2, "conditioning_embedding_channels": 16})
    with pytest.raises(NotImplementedError, match="input_hint_block"):
        j({"num_layers": 2, "conditioning_embedding_channels": 16})
    with pytest.raises(ValueError, match="in_channels = 128, out_channels = 64"):
        j({"in_channels": 128, "out_channels": 64})
    with pytest.raises(ValueError, match="num_layers = 0"):
        j({"num_layers": 0})
    with pytest.raises(Exception, match="HIP engine only"):
        FluxControlNetModel(FluxControlNetConfig(num_layers=1, num_single_layers=0), device="cpu")


def _host_controlnet(**cfg):
    """No GPU: a FluxControlNetModel that carries only its config (what the pipeline reads before the first device call)."""
    from thinkdiff.models import FluxControlNetConfig, FluxControlNetModel
    m = object.__new__(FluxControlNetModel)
    m.config = FluxControlNetConfig(**{**dict(num_layers=2, num_single_layers=1, num_attention_heads=4, joint_attention_dim=32,
                                              pooled_projection_dim=16, guidance_embeds=False), **cfg})
    return m


def _stub(controlnet, **tr_cfg):
    from thinkdiff.models import FluxControlNetPipelineRewritePrompt, FluxTransformerConfig
    tr = SimpleNamespace(device=torch.device("cpu"), dtype=BF, list_adapters=lambda: [],
                         config=FluxTransformerConfig(**{**dict(num_attention_heads=4, joint_attention_dim=32, pooled_projection_dim=16), **tr_cfg}))
    return FluxControlNetPipelineRewritePrompt(transformer=tr, controlnet=controlnet)


def _embeds():
    return dict(prompt_embeds=torch.zeros(2, 8, 32, dtype=BF), pooled_prompt_embeds=torch.zeros(2, 16, dtype=BF), height=64, width=64, num_inference_steps=4)


def test_model_refuses_what_the_side_network_does_not_take():
    m = _host_controlnet()
    for call, word in ((lambda: m.set_precision("int8"), "int8"), (lambda: m.set_precision("fp8"), "fp8"), (lambda: m.set_attention("fp8"), "fp8"),
                       (lambda: m.load_lora_adapter({}), "load_lora_adapter"), (lambda: m.attach_controlnet(m), "attach_controlnet"),
                       (lambda: m.forward_step(None, 0), "no velocity")):
        with pytest.raises(NotImplementedError, match=word):
            call()
    with pytest.raises(ValueError, match="control_mode = 1"):
        m.set_condition(None, None, None, control_mode=1)
    with pytest.raises(ValueError, match="num_mode = 3"):
        _host_controlnet(num_mode=3).set_condition(None, None, None)


def test_pipeline_refusals():
    from PIL import Image
    from thinkdiff.models import FluxControlNetPipelineRewritePrompt
    cn = _host_controlnet()
    p = _stub(cn)
    img = Image.new("RGB", (64, 64))
    kw = _embeds()
    for name, val in (("callback_on_step_end", lambda *a: {}), ("sigmas", [1.0, 0.5]), ("joint_attention_kwargs", {"scale": 0.5})):
        with pytest.raises(NotImplementedError, match=name):
            p(control_image=img, **{name: val}, **kw)
    with pytest.raises(NotImplementedError, match="generator"):
        p(control_image=img, generator=[torch.Generator()], **kw)
    # lists of ControlNets, and the per-ControlNet lists that go with them
    with pytest.raises(NotImplementedError, match="list of 2 ControlNets"):
        _stub([cn, cn])
    p.controlnet = [cn, cn]
    with pytest.raises(NotImplementedError, match="FluxMultiControlNetModel"):
        p(control_image=img, **kw)
    p.controlnet = cn
    for name, val in (("controlnet_conditioning_scale", [0.5, 0.7]), ("control_guidance_start", [0.0, 0.1]), ("control_guidance_end", [0.9, 1.0]),
                      ("control_mode", [0, 1])):
        with pytest.raises(NotImplementedError, match=name):
            p(control_image=img, **{name: val}, **kw)
    with pytest.raises(NotImplementedError, match="list of lists"):
        p(control_image=[[img], [img]], **kw)
    # the union rule, both ways
    with pytest.raises(ValueError, match="control_mode = 1"):
        p(control_image=img, control_mode=1, **kw)
    u = _stub(_host_controlnet(num_mode=4))
    with pytest.raises(ValueError, match="num_mode = 4.*control_mode is required"):
        u(control_image=img, **kw)
    with pytest.raises(ValueError, match="control_mode = 4 outside the 4 modes"):
        u(control_image=img, control_mode=4, **kw)
    # arguments
    with pytest.raises(ValueError, match="control_guidance_start = 0.8 exceeds control_guidance_end = 0.5"):
        p(control_image=img, control_guidance_start=0.8, control_guidance_end=0.5, **kw)
    with pytest.raises(ValueError, match="multiples of 16"):
        p(control_image=img, **{**kw, "width": 40})
    with pytest.raises(ValueError, match="control_image"):
        p(**kw)
    with pytest.raises(ValueError, match="prompt"):
        p(control_image=img, height=64, width=64)
    with pytest.raises(ValueError, match="3 control images"):
        p(control_image=[img] * 3, **kw)
    with pytest.raises(ValueError, match="taken as latents"):
        p(control_image=torch.zeros(1, 16, 4, 8), **kw)
    with pytest.raises(ValueError, match="not resized"):
        p(control_image=torch.zeros(1, 3, 32, 64), **kw)
    with pytest.raises(ValueError, match="packed"):
        p(control_image=img, latents=torch.zeros(2, 16, 8, 8), **kw)
    with pytest.raises(ValueError, match="FluxControlNetModel"):
        _stub(None)(control_image=img, **kw)
    # a ControlNet on a channel-conditioned transformer, and mismatched widths
    with pytest.raises(NotImplementedError, match="in_channels = 128, out_channels = 64"):
        _stub(cn, in_channels=128, out_channels=64)(control_image=img, **kw)
    with pytest.raises(ValueError, match="inner width 512.*inner width 1024"):
        _stub(_host_controlnet(num_attention_heads=8))(control_image=img, **kw)
    assert isinstance(p, FluxControlNetPipelineRewritePrompt)


# ---- optional pin against diffusers ---------------------------------------------------------------------------------------------------------
def test_pin_against_diffusers_if_present():
    try:
        import diffusers
        model_cls = diffusers.FluxControlNetModel
    except Exception as e:  # noqa: BLE001
        print(f"diffusers: absent ({type(e).__name__}: {e})")
        pytest.skip("diffusers: absent -- tests/controlnet_common.py stays 'parity unpinned'")
    cfg_cn = C.cn_config(2, 3)
    sd_cn = _cast(C.cn_init_weights(cfg_cn, 2, seed=C.SEED_CN), torch.float32)
    try:
        m = model_cls(patch_size=1, in_channels=64, num_layers=2, num_single_layers=3, attention_head_dim=128, num_attention_heads=cfg_cn.num_attention_heads,
                      joint_attention_dim=cfg_cn.joint_attention_dim, pooled_projection_dim=cfg_cn.pooled_projection_dim, guidance_embeds=False,
                      axes_dims_rope=tuple(cfg_cn.axes_dims_rope), num_mode=2).eval()
        missing, unexpected = m.load_state_dict(sd_cn, strict=False)
    except (TypeError, AttributeError, ImportError) as e:
        pytest.skip(f"diffusers {diffusers.__version__} is present but its API differs ({type(e).__name__}: {e}); the restatement stays unpinned")
    assert not missing and not unexpected, (missing, unexpected)
    lat, cond, _, pe, pool = C.inputs(cfg_cn, C.H2 * C.W2, C.T_TXT, C.SEED_IN)
    x, e, p, t, ids, tids, _ = _call_args(cfg_cn, lat, pe, pool, torch.float32)
    with torch.no_grad():
        want = m(hidden_states=x, controlnet_cond=cond[None].float(), controlnet_mode=torch.tensor([[1]]), conditioning_scale=C.SCALE, encoder_hidden_states=e,
                 pooled_projections=p, timestep=t, img_ids=ids, txt_ids=tids, guidance=None, return_dict=False)
    got = C.controlnet_forward_ref(sd_cn, cfg_cn, x, cond[None].float(), 1, e, p, t, ids, tids, None, C.SCALE)
    for w, g in zip(list(want[0]) + list(want[1] or []), got[0] + got[1]):
        assert float((g - w).abs().max() / w.abs().max()) < 1e-4
