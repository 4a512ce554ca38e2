"""FLUX IP-Adapter without a GPU: the properties of the test fixture (tests/ip_adapter_common.py), the reference's identity with the oracle, the
checkpoint key conversion, the scale expansion and every Python-side refusal."""
import ctypes
import os

import pytest
import torch

import ip_adapter_common as C
from oracle import flux_ref as R
from thinkdiff.models import flux_ip_adapter as ipa

BF = torch.bfloat16
S = C.H2 * C.W2


@pytest.fixture(scope="module")
def fx():
    cfg = C.main_config()
    sd = R.init_weights(cfg, seed=C.SEED_MAIN)
    lat, pe, pool = C.inputs(cfg, S, C.T_TXT)
    out = dict(cfg=cfg, sd=sd, lat=lat, pe=pe, pool=pool)

    def fwd(dtype, specs):
        w = {k: v.to(dtype) for k, v in sd.items()}
        return C.transformer_forward_ref(w, cfg, *C.step_args(lat, pe, pool, dtype, S, C.T_TXT), adapters=C.make_adapters(cfg, specs, dtype))

    out["fwd"] = fwd
    out["plain16"], out["plain32"] = fwd(BF, []), fwd(torch.float32, [])
    return out


@pytest.mark.parametrize("num_tokens", [4, 16])
def test_fixture_properties(fx, num_tokens):
    """The image prompt moves the output, another image moves it again, and the reference's own bf16 error stays the plain model's."""
    ip = C.ip_init_weights(fx["cfg"], num_tokens)
    e1, e2 = C.image_embeds(1, 100), C.image_embeds(1, 101)
    v16, v32 = fx["fwd"](BF, [(ip, e1, C.SCALE)]), fx["fwd"](torch.float32, [(ip, e1, C.SCALE)])
    other = fx["fwd"](BF, [(ip, e2, C.SCALE)])
    d_plain, d_other = C.rel_rmse(fx["plain16"], v16), C.rel_rmse(other, v16)
    e_ip, e_plain = C.rel_rmse(v16, v32), C.rel_rmse(fx["plain16"], fx["plain32"])
    print(f"{num_tokens} tokens: IP vs plain {d_plain:.3f}  other image {d_other:.3f}  bf16~fp32 with IP {e_ip:.4f}  plain {e_plain:.4f}")
    assert d_plain >= 0.1 and d_other >= 0.1
    assert e_ip <= 1.2 * e_plain


def test_reference_is_the_oracle_without_a_contribution(fx):
    """No adapter, zero to_v_ip (weight and bias) and scale 0: R.transformer_forward, to bits."""
    cfg = fx["cfg"]
    args = C.step_args(fx["lat"], fx["pe"], fx["pool"], BF, S, C.T_TXT)
    want = R.transformer_forward(fx["sd"], cfg, *args)
    assert torch.equal(fx["plain16"], want)
    ip = C.ip_init_weights(cfg, 4)
    zero_v = {"image_proj": ip["image_proj"], "ip_adapter": {k: (torch.zeros_like(v) if "to_v_ip" in k else v) for k, v in ip["ip_adapter"].items()}}
    assert torch.equal(fx["fwd"](BF, [(zero_v, C.image_embeds(1, 100), C.SCALE)]), want)
    assert torch.equal(fx["fwd"](BF, [(ip, C.image_embeds(1, 100), 0.0)]), want)
    # a per-block scale [0, s] skips block 0 and differs from both
    v_blk = fx["fwd"](BF, [(ip, C.image_embeds(1, 100), [0.0, C.SCALE])])
    assert not torch.equal(v_blk, want) and not torch.equal(v_blk, fx["fwd"](BF, [(ip, C.image_embeds(1, 100), C.SCALE)]))


def test_image_projection_shapes(fx):
    cfg = fx["cfg"]
    ip = C.ip_init_weights(cfg, 16)
    t = C.image_tokens(ip, cfg, C.image_embeds(2, 3))
    assert t.shape == (32, cfg.joint_attention_dim) and t.dtype == BF
    k, v = C.block_kv(ip, 1, t)
    assert k.shape == v.shape == (32, cfg.inner_dim)


# ---- checkpoint keys ----------------------------------------------------------------------------------------------------------------------
def _load(sd, cfg, **kw):
    return ipa.load_ip_adapter_state_dict(sd, num_layers=cfg.num_layers, joint_dim=cfg.joint_attention_dim, inner_dim=cfg.inner_dim, **kw)


def test_key_conversion_round_trip(fx):
    cfg = fx["cfg"]
    ip = C.ip_init_weights(cfg, 4)
    x = ipa.diffusers_to_xlabs(ip)
    assert "ip_adapter_proj_model.proj.weight" in x and "double_blocks.1.processor.ip_adapter_double_stream_v_proj.bias" in x
    assert len(x) == 4 + 4 * cfg.num_layers
    back = ipa.xlabs_to_diffusers(x)
    assert set(back) == {"image_proj", "ip_adapter"}
    for part in back:
        assert set(back[part]) == set(ip[part]) and all(back[part][k] is ip[part][k] for k in ip[part])
    flat_d, nt, E = _load(ip, cfg)
    flat_x, nt_x, E_x = _load(x, cfg)
    assert (nt, E) == (nt_x, E_x) == (4, C.E_DIM)
    assert set(flat_d) == set(flat_x) and all(flat_d[k] is flat_x[k] for k in flat_d)
    assert "image_proj.norm.bias" in flat_d and "ip_adapter.1.to_k_ip.weight" in flat_d


def test_file_forms(fx, tmp_path):
    from safetensors.torch import save_file
    cfg = fx["cfg"]
    x = {k: v.contiguous() for k, v in ipa.diffusers_to_xlabs(C.ip_init_weights(cfg, 4)).items()}
    save_file(x, str(tmp_path / "ip_adapter.safetensors"))
    a, nt, _ = _load(str(tmp_path / "ip_adapter.safetensors"), cfg)
    b, _, _ = _load(str(tmp_path), cfg, weight_name="ip_adapter.safetensors")
    assert nt == 4 and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError, match="weight_name"):
        _load(str(tmp_path), cfg)
    with pytest.raises(FileNotFoundError, match="hub ids cannot be fetched"):
        _load("XLabs-AI/flux-ip-adapter", cfg)


def test_loader_refusals_name_the_key(fx):
    cfg = fx["cfg"]
    ip = C.ip_init_weights(cfg, 4)
    x = ipa.diffusers_to_xlabs(ip)
    with pytest.raises(KeyError, match="single_blocks.0.foo"):
        _load({**x, "single_blocks.0.foo": torch.zeros(1)}, cfg)
    with pytest.raises(KeyError, match="image_proj.extra"):
        _load({"image_proj": {**ip["image_proj"], "extra": torch.zeros(1)}, "ip_adapter": ip["ip_adapter"]}, cfg)
    with pytest.raises(KeyError, match="ip_adapter.0.to_q_ip.weight"):
        _load({"image_proj": ip["image_proj"], "ip_adapter": {**ip["ip_adapter"], "0.to_q_ip.weight": torch.zeros(1)}}, cfg)
    # wrong block count: one too many, one missing
    three = C.ip_init_weights(R.tiny_config(num_layers=3, num_single_layers=1), 4)
    with pytest.raises(ValueError, match="double block 2, the transformer has 2"):
        _load(three, cfg)
    short = {"image_proj": ip["image_proj"], "ip_adapter": {k: v for k, v in ip["ip_adapter"].items() if not k.startswith("1.")}}
    with pytest.raises(ValueError, match="missing key 'ip_adapter.1.to_k_ip.weight'"):
        _load(short, cfg)
    # wrong J, wrong D
    with pytest.raises(ValueError, match="image_proj.proj.weight.*J = joint_attention_dim = 768"):
        ipa.load_ip_adapter_state_dict(ip, num_layers=2, joint_dim=768, inner_dim=512)
    with pytest.raises(ValueError, match="ip_adapter.0.to_k_ip.weight.*expected \\(1024, 512\\)"):
        ipa.load_ip_adapter_state_dict(ip, num_layers=2, joint_dim=512, inner_dim=1024)
    bad = {"image_proj": {**ip["image_proj"], "norm.weight": torch.zeros(100)}, "ip_adapter": ip["ip_adapter"]}
    with pytest.raises(ValueError, match="image_proj.norm.weight"):
        _load(bad, cfg)


# ---- scales and embeds --------------------------------------------------------------------------------------------------------------------
def test_scale_expansion():
    assert ipa.expand_scales(0.5, 2, 3) == [[0.5] * 3, [0.5] * 3]
    assert ipa.expand_scales([0.7, 0.4], 2, 2) == [[0.7, 0.7], [0.4, 0.4]]
    assert ipa.expand_scales([[0.0, 0.7], 1], 2, 2) == [[0.0, 0.7], [1.0, 1.0]]
    with pytest.raises(ValueError, match="1 scales for 2 loaded adapters"):
        ipa.expand_scales([0.7], 2, 2)
    with pytest.raises(ValueError, match="adapter 0: 3 per-block scales, the transformer has 2 double blocks"):
        ipa.expand_scales([[0.1, 0.2, 0.3]], 1, 2)


def test_image_embeds_normalisation():
    e = torch.zeros(2, 32)
    out = ipa.normalize_image_embeds(e, 1, 3, [32])
    assert len(out) == 1 and out[0].shape == (1, 2, 32)
    out = ipa.normalize_image_embeds([torch.zeros(3, 1, 32), torch.zeros(4, 48)], 2, 3, [32, 48])
    assert out[0].shape == (3, 1, 32) and out[1].shape == (1, 4, 48)
    with pytest.raises(ValueError, match="2 entries for 1 loaded adapters"):
        ipa.normalize_image_embeds([e, e], 1, 1, [32])
    with pytest.raises(ValueError, match="width 32, adapter 0 projects embeddings of width 64"):
        ipa.normalize_image_embeds(e, 1, 1, [64])
    with pytest.raises(ValueError, match="batch 2, the call has 3 prompts"):
        ipa.normalize_image_embeds(torch.zeros(2, 1, 32), 1, 3, [32])
    with pytest.raises(ValueError, match="must be a tensor"):
        ipa.normalize_image_embeds([torch.zeros(32)], 1, 1, [32])


class _NoAdapters:
    def ip_adapters(self):
        return []


def test_pipeline_refusals_without_an_engine():
    """The base pipeline's IP keywords: an error instead of a picture that never saw the image prompt."""
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    pipe = FluxPipelineRewritePrompt(transformer=_NoAdapters())
    e = torch.zeros(1, 1, 32)
    assert pipe._ip_call_embeds(1, None, None, None, None) is None
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe._ip_call_embeds(1, None, e, None, None)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe._ip_call_embeds(1, object(), None, None, None)
    for neg in ((e, None), (None, e)):
        with pytest.raises(NotImplementedError, match="negative_ip_adapter_image"):
            pipe._ip_call_embeds(1, None, e, *neg)
    with pytest.raises(ValueError, match="ip_adapter_image_embeds"):
        pipe.encode_image(torch.zeros(1, 3, 8, 8))           # no image encoder: the message names the embeds keyword

    class Enc(torch.nn.Module):
        def forward(self, x):
            from types import SimpleNamespace
            return SimpleNamespace(image_embeds=x.flatten(1)[:, :32])

    pipe.image_encoder, pipe.feature_extractor = Enc(), None
    assert pipe.encode_image(torch.zeros(2, 3, 8, 8)).shape == (2, 32)
    with pytest.raises(ValueError, match="feature_extractor"):
        pipe.encode_image(object())


def test_kontext_keeps_refusing_the_keywords():
    from thinkdiff.models import flux_kontext
    for k in ("ip_adapter_image", "ip_adapter_image_embeds", "negative_ip_adapter_image", "negative_ip_adapter_image_embeds"):
        assert k in flux_kontext.REFUSED_ARGS


def test_c_abi_refusals_without_a_gpu():
    """td_ip_attention_bf16's argument errors come back as TD_ERR_INVALID before any HIP call, the offender named."""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so"))
    lib.td_last_error.restype = ctypes.c_char_p
    assert lib.td_abi_version() >= 5
    one = ctypes.c_void_p(256)
    i64, f32 = ctypes.c_int64, ctypes.c_float

    def call(q=one, ldq=1536, n_keys=4, rows=64, H=4, ldkv=512, ldo=512, w=None):
        return lib.td_ip_attention_bf16(q, i64(ldq), one, one, i64(ldkv), one, i64(ldo), rows, H, n_keys, w, f32(1e-6), f32(0.7), 0, None)

    for kw, word in ((dict(n_keys=0), b"n_keys=0"), (dict(n_keys=257), b"n_keys=257"), (dict(q=ctypes.c_void_p(258)), b"q must be 16-byte aligned"),
                     (dict(ldq=1540), b"ldq=1540"), (dict(ldq=256), b"ldq=256"), (dict(rows=0), b"rows=0"), (dict(H=0), b"H=0"),
                     (dict(ldkv=500), b"ldkv=500"), (dict(ldo=504), b"ldo=504"), (dict(w=ctypes.c_void_p(264)), b"norm_w"), (dict(q=None), b"null")):
        assert call(**kw) == 2 and word in lib.td_last_error(), (kw, lib.td_last_error())
    assert lib.td_flux_set_ip_image_embeds(None, 0, None, 0, None) == 2
    assert lib.td_flux_ip_adapter_add(None, 4, 32, None) == 2
