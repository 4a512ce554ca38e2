"""Several FLUX ControlNets on one transformer, without a GPU: identities of the test-local reference (tests/multi_controlnet_common.py),
the per-net keep and scale tables, the sensitivity the GPU tests rely on, the refusals of `FluxMultiControlNetModel` and of the pipeline
(before the first device call) and the new C entries' argument errors (TD_ERR_INVALID before any HIP call)."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import controlnet_common as C
import multi_controlnet_common as M
from oracle import flux_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
BF = torch.bfloat16
S = C.H2 * C.W2


def _args(lat, pe, pool, dtype):
    t = torch.tensor([0.61]).bfloat16() if dtype == BF else torch.tensor([0.61]).bfloat16().float()
    ids, tids = R.latent_image_ids(C.H2, C.W2).to(dtype), torch.zeros(pe.shape[0], 3).to(dtype)
    return lat[None].to(dtype), pe[None].to(dtype), pool[None].to(dtype), t, ids, tids, torch.tensor([3.5])


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


@pytest.fixture(scope="module")
def world():
    cfg = C.main_config()
    lat, cond, cond2, pe, pool = C.inputs(cfg, S, C.T_TXT, C.SEED_IN)
    w = dict(cfg=cfg, sd=R.init_weights(cfg, seed=C.SEED_MAIN), lat=lat, cond=cond, cond2=cond2, pe=pe, pool=pool, cn={})
    for (case, _, _), seed in zip(M.NETS, (C.SEED_CN, M.SEED_CN2)):
        n_d, n_s, num_mode, mode = C.CASES[case]
        cc = C.cn_config(n_d, n_s)
        w["cn"][case] = dict(cfg=cc, sd=C.cn_init_weights(cc, num_mode, seed=seed), mode=mode)
    return w


def _nets(w, dtype, conds=("cond", "cond2"), scales=(0.7, 0.45)):
    return [M.net(_cast(w["cn"][case]["sd"], dtype), w["cn"][case]["cfg"], w[cd][None].to(dtype), w["cn"][case]["mode"], sc)
            for (case, _, _), cd, sc in zip(M.NETS, conds, scales)]


# ---- reference identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("which", [0, 1])
def test_one_net_is_the_single_net_reference_bit_for_bit(world, which, dtype):
    """K = 1 equals controlled_forward_ref; so does K = 2 with the other net at scale 0 (a net at scale 0 is left out)."""
    w = world
    sd = _cast(w["sd"], dtype)
    x, e, p, t, ids, tids, g = _args(w["lat"], w["pe"], w["pool"], dtype)
    nets = _nets(w, dtype)
    n = nets[which]
    want = C.controlled_forward_ref(sd, w["cfg"], n["sd"], n["cfg"], x, n["cond"], n["mode"], e, p, t, ids, tids, g, n["scale"])
    assert torch.equal(M.multi_controlled_forward_ref(sd, w["cfg"], [n], x, e, p, t, ids, tids, g), want)
    off = [nk if k == which else {**nk, "scale": 0.0} for k, nk in enumerate(nets)]
    assert torch.equal(M.multi_controlled_forward_ref(sd, w["cfg"], off, x, e, p, t, ids, tids, g), want)
    plain = R.transformer_forward(sd, w["cfg"], x, e, p, t, ids, tids, g)
    assert not torch.equal(want, plain)
    assert torch.equal(M.multi_controlled_forward_ref(sd, w["cfg"], [{**nk, "scale": 0.0} for nk in nets], x, e, p, t, ids, tids, g), plain)
    assert torch.equal(M.multi_controlled_forward_ref(sd, w["cfg"], [], x, e, p, t, ids, tids, g), plain)


def test_the_fold_is_not_two_successive_injections():
    """bf16(h + bf16(a + b)) against bf16(bf16(h + a) + b): different values on spread data, which is why the sum needs its own kernel."""
    g = torch.Generator().manual_seed(5)
    h, a, b = (torch.randn(8192, generator=g).bfloat16() for _ in range(3))
    assert torch.equal(M.fold([a, b]), a + b) and M.fold([]) is None and M.fold([a]) is a
    assert not torch.equal(h + M.fold([a, b]), (h + a) + b)
    # a left fold: ((a + b) + c), not (a + (b + c))
    c = torch.randn(8192, generator=g).bfloat16()
    assert torch.equal(M.fold([a, b, c]), (a + b) + c) and not torch.equal(M.fold([a, b, c]), a + (b + c))


def test_reference_is_sensitive_to_each_net_and_to_which_image_goes_where(world):
    """With the seeds and scales of the GPU test: dropping either net, or swapping the two control images, moves the output by > 0.05."""
    w = world
    x, e, p, t, ids, tids, g = _args(w["lat"], w["pe"], w["pool"], BF)
    run = lambda **kw: M.multi_controlled_forward_ref(w["sd"], w["cfg"], _nets(w, BF, **kw), x, e, p, t, ids, tids, g)
    both = run()
    d = dict(drop1=C.rel_rmse(run(scales=(0.7, 0.0)), both), drop0=C.rel_rmse(run(scales=(0.0, 0.45)), both),
             swap=C.rel_rmse(run(conds=("cond2", "cond")), both), none=C.rel_rmse(run(scales=(0.0, 0.0)), both))
    print(" ".join(f"{k} {v:.3f}" for k, v in d.items()))
    assert all(v > 0.05 for v in d.values())


# ---- keep and scale tables ----------------------------------------------------------------------------------------------------------------
def test_keep_and_scale_tables_for_list_and_scalar_arguments():
    from thinkdiff.models.flux_controlnet import controlnet_scale_tables
    assert M.keep_tables(4, 2) == [[1.0] * 4, [1.0] * 4]
    assert M.keep_tables(4, 2, [0.0, 0.25], [0.5, 1.0]) == [[1, 1, 0, 0], [0, 1, 1, 1]]
    assert M.keep_tables(4, 3, 0.25, [0.5, 0.75, 1.0]) == [[0, 1, 0, 0], [0, 1, 1, 0], [0, 1, 1, 1]]
    for kw in (dict(), dict(scale=0.7), dict(scale=[0.7, 0.45]), dict(scale=[0.7, 0.45], start=[0.0, 0.25], end=[0.5, 1.0]), dict(scale=0.5, end=[0.25, 1.0])):
        want = M.scale_tables(4, 2, **kw)
        got = controlnet_scale_tables(4, 2, kw.get("scale", 1.0), kw.get("start", 0.0), kw.get("end", 1.0))
        assert got == want, kw
    assert controlnet_scale_tables(4, 2, [0.7, 0.45], [0.0, 0.25], [0.5, 1.0]) == [[0.7, 0.7, 0.0, 0.0], [0.0, 0.45, 0.45, 0.45]]
    assert controlnet_scale_tables(3, 1, 0.7, 0.0, 0.7) == [[0.7 * k for k in C.keep_schedule(3, 0.0, 0.7)]]
    for bad in (dict(conditioning_scale=[1.0]), dict(start=[0.0, 0.0, 0.0]), dict(end=[1.0])):
        with pytest.raises(ValueError, match="for 2 ControlNets"):
            controlnet_scale_tables(4, 2, **bad)


# ---- Python refusals ----------------------------------------------------------------------------------------------------------------------
def _host_controlnet(**cfg):
    """No GPU: a FluxControlNetModel that carries only its config (what the pipeline reads before the first device call)."""
    from thinkdiff.models import FluxControlNetConfig, FluxControlNetModel
    m = object.__new__(FluxControlNetModel)
    m.config = FluxControlNetConfig(**{**dict(num_layers=2, num_single_layers=1, num_attention_heads=4, joint_attention_dim=32,
                                              pooled_projection_dim=16, guidance_embeds=False), **cfg})
    return m


def _stub(controlnet):
    from thinkdiff.models import FluxControlNetPipelineRewritePrompt, FluxTransformerConfig
    tr = SimpleNamespace(device=torch.device("cpu"), dtype=BF, list_adapters=lambda: [],
                         config=FluxTransformerConfig(num_attention_heads=4, joint_attention_dim=32, pooled_projection_dim=16))
    return FluxControlNetPipelineRewritePrompt(transformer=tr, controlnet=controlnet)


def test_multi_model_refusals():
    from thinkdiff.models import FluxMultiControlNetModel
    cn = _host_controlnet()
    m = FluxMultiControlNetModel([cn, cn])      # the same model twice is a list of two
    assert len(m) == 2 and m[0] is cn and list(m) == [cn, cn]
    assert len(FluxMultiControlNetModel(cn)) == 1 and len(FluxMultiControlNetModel([cn] * 4)) == 4
    with pytest.raises(ValueError, match="1 to 4 ControlNets, got 5"):
        FluxMultiControlNetModel([cn] * 5)
    with pytest.raises(ValueError, match="1 to 4 ControlNets, got 0"):
        FluxMultiControlNetModel([])
    with pytest.raises(ValueError, match="entry 1 is a str"):
        FluxMultiControlNetModel([cn, "canny"])


def test_pipeline_refusals_with_a_multi_model():
    from PIL import Image
    from thinkdiff.models import FluxMultiControlNetModel
    cn, un = _host_controlnet(), _host_controlnet(num_mode=4)
    img = Image.new("RGB", (64, 64))
    kw = dict(prompt_embeds=torch.zeros(2, 8, 32, dtype=BF), pooled_prompt_embeds=torch.zeros(2, 16, dtype=BF), height=64, width=64, num_inference_steps=4)
    p = _stub(FluxMultiControlNetModel([cn, un]))
    ok = dict(control_image=[img, img], control_mode=[None, 1])
    # wrong lengths, each naming its keyword and both counts
    for name, val in (("control_image", [img]), ("control_image", [img] * 3), ("control_mode", [1]), ("controlnet_conditioning_scale", [0.5]),
                      ("control_guidance_start", [0.0, 0.1, 0.2]), ("control_guidance_end", [1.0])):
        with pytest.raises(ValueError, match=f"{name} has {len(val)} entries for 2 ControlNets"):
            p(**{**ok, name: val}, **kw)
    with pytest.raises(ValueError, match="control_image must be a list of 2"):
        p(**{**ok, "control_image": img}, **kw)
    with pytest.raises(ValueError, match="control_mode = 1 must be a list of 2"):
        p(**{**ok, "control_mode": 1}, **kw)
    with pytest.raises(ValueError, match="control_image"):
        p(control_mode=[None, 1], **kw)
    # the union rule, per net and naming the net
    with pytest.raises(ValueError, match="ControlNet 1 of 2.*num_mode = 4.*control_mode is required"):
        p(control_image=[img, img], **kw)
    with pytest.raises(ValueError, match="ControlNet 1 of 2.*control_mode is required"):
        p(control_image=[img, img], control_mode=[None, None], **kw)
    with pytest.raises(ValueError, match="ControlNet 0 of 2: control_mode = 2 on a ControlNet without a mode embedder"):
        p(control_image=[img, img], control_mode=[2, 1], **kw)
    with pytest.raises(ValueError, match="ControlNet 1 of 2: control_mode = 4 outside the 4 modes"):
        p(control_image=[img, img], control_mode=[None, 4], **kw)
    with pytest.raises(ValueError, match="ControlNet 1 of 2: control_guidance_start = 0.8 exceeds control_guidance_end = 0.5"):
        p(control_guidance_start=[0.0, 0.8], control_guidance_end=[1.0, 0.5], **ok, **kw)
    with pytest.raises(ValueError, match="3 control images of ControlNet 1"):
        p(control_image=[img, [img] * 3], control_mode=[None, 1], **kw)
    with pytest.raises(ValueError, match=r"control_image\[1\]: a 16-channel control_image is taken as latents"):
        p(control_image=[img, torch.zeros(1, 16, 4, 8)], control_mode=[None, 1], **kw)
    # more than 4 nets: the wrapper refuses them, and so does the pipeline should a list grow behind its back
    m = FluxMultiControlNetModel([cn] * 4)
    m.nets.append(cn)
    with pytest.raises(ValueError, match="5 ControlNets.*1 to 4"):
        _stub(m)(control_image=[img] * 5, **kw)
    # the raw list and the single-net forms point at the wrapper
    with pytest.raises(NotImplementedError, match=r"list of 2 ControlNets.*FluxMultiControlNetModel\(\[\.\.\.\]\)"):
        _stub([cn, cn])
    with pytest.raises(NotImplementedError, match=r"controlnet_conditioning_scale.*FluxMultiControlNetModel\(\[\.\.\.\]\)"):
        _stub(cn)(control_image=img, controlnet_conditioning_scale=[0.5, 0.7], **kw)
    with pytest.raises(NotImplementedError, match=r"list of lists.*FluxMultiControlNetModel\(\[\.\.\.\]\)"):
        _stub(cn)(control_image=[[img], [img]], **kw)


# ---- the C ABI refuses bad arguments before any HIP call ------------------------------------------------------------------------------------
def _lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.td_flux_residual_inject_multi_bf16.argtypes = [vp, i64, vp, vp, vp, i32, i32, i32, vp]
    lib.td_flux_attach_controlnets.argtypes = [vp, vp, i32]
    lib.td_flux_set_controlnet_scales_at.argtypes = [vp, i32, vp, i32]
    lib.td_flux_attached_controlnets.argtypes = [vp, vp]
    return lib


def test_abi_version_names_the_multi_controlnet():
    assert _lib().td_abi_version() >= 10


def test_multi_inject_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    h, r0 = 1 << 20, 1 << 22      # never dereferenced: every check precedes the launch

    def inj(h=h, ldh=64, r=None, ldr=None, scales=None, n=2, rows=4, D=64, null=()):
        r = [r0, r0 + (1 << 16), r0 + (2 << 16), r0 + (3 << 16), r0 + (4 << 16)][:max(n, 1)] if r is None else r
        ra = (ctypes.c_void_p * len(r))(*r)
        la = (ctypes.c_int64 * len(r))(*(ldr or [64] * len(r)))
        sa = (ctypes.c_float * len(r))(*(scales or [0.7] * len(r)))
        a = dict(h=h, r=ctypes.cast(ra, ctypes.c_void_p), ldr=ctypes.cast(la, ctypes.c_void_p), scales=ctypes.cast(sa, ctypes.c_void_p))
        a.update({k: None for k in null})
        return lib.td_flux_residual_inject_multi_bf16(a["h"], ldh, a["r"], a["ldr"], a["scales"], n, rows, D, None), lib.td_last_error()

    for null in ("h", "r", "ldr", "scales"):
        rc, msg = inj(null=(null,))
        assert rc == 2 and b"null" in msg, null
    rc, msg = inj(r=[r0, 0])
    assert rc == 2 and b"r[1] is null" in msg
    rc, msg = inj(n=5)
    assert rc == 2 and b"n=5 outside 1 .. 4" in msg
    rc, msg = inj(n=0)
    assert rc == 2 and b"n=0 outside 1 .. 4" in msg
    rc, msg = inj(D=60)
    assert rc == 2 and b"D=60" in msg and b"multiple of 8" in msg
    rc, msg = inj(r=[r0, r0 + (1 << 16) + 2])
    assert rc == 2 and b"r[1] must be 16-byte aligned" in msg
    rc, msg = inj(h=h + 8)
    assert rc == 2 and b"h must be 16-byte aligned" in msg
    rc, msg = inj(ldr=[64, 56])
    assert rc == 2 and b"ldr[1]=56" in msg and b"at least D" in msg
    rc, msg = inj(ldr=[68, 64])
    assert rc == 2 and b"ldr[0]=68" in msg and b"multiple of 8" in msg
    rc, msg = inj(ldh=68)
    assert rc == 2 and b"ldh=68" in msg
    rc, msg = inj(rows=0)
    assert rc == 2
    # overlap with h (updated in place): the second, then the third operand; touching h's end is allowed to pass this check
    rc, msg = inj(r=[r0, h + 64])
    assert rc == 2 and b"r[1] must not overlap h" in msg
    rc, msg = inj(n=3, r=[r0, r0 + (1 << 16), h])
    assert rc == 2 and b"r[2] must not overlap h" in msg
    rc, msg = inj(r=[h, r0])
    assert rc == 2 and b"r[0] must not overlap h" in msg
    rc, msg = inj(ldh=1 << 40)
    assert rc == 2 and b"32-bit" in msg
    rc, msg = inj(ldr=[64, 1 << 40])
    assert rc == 2 and b"ldr[1]" in msg and b"32-bit" in msg
    # a scale that is not finite is refused, naming k (td_flux_set_controlnet_scales refuses the same)
    for bad in (float("nan"), float("inf")):
        rc, msg = inj(scales=[0.7, bad])
        assert rc == 2 and b"scales[1] is not finite" in msg


def test_multi_attach_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib()
    f, a, b = 1 << 20, 1 << 21, 1 << 22      # never dereferenced: the list is checked before any context is looked into
    lst = lambda *p: ctypes.cast((ctypes.c_void_p * max(1, len(p)))(*p), ctypes.c_void_p)
    one = ctypes.cast((ctypes.c_float * 1)(1.0), ctypes.c_void_p)
    n = ctypes.c_int(-1)
    assert lib.td_flux_attach_controlnets(None, lst(a), 1) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_attach_controlnets(f, None, 2) == 2 and b"null list of 2" in lib.td_last_error()
    assert lib.td_flux_attach_controlnets(f, lst(a, b, a, b, a), 5) == 2 and b"n=5 ControlNets outside 0 .. 4" in lib.td_last_error()
    assert lib.td_flux_attach_controlnets(f, lst(a), -1) == 2 and b"n=-1" in lib.td_last_error()
    assert lib.td_flux_attach_controlnets(f, lst(a, None), 2) == 2 and b"ControlNet context 1 of 2 is null" in lib.td_last_error()
    assert lib.td_flux_attach_controlnets(f, lst(a, a), 2) == 2 and b"entries 0 and 1 are the same ControlNet context" in lib.td_last_error()
    assert lib.td_flux_attach_controlnets(f, lst(a, b, a), 3) == 2 and b"entries 0 and 2 are the same ControlNet context" in lib.td_last_error()
    assert lib.td_flux_set_controlnet_scales_at(None, 0, one, 1) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_set_controlnet_scales_at(f, 0, None, 1) == 2 and b"null" in lib.td_last_error()
    assert lib.td_flux_set_controlnet_scales_at(f, 4, one, 1) == 2 and b"ControlNet 4 outside 0 .. 3" in lib.td_last_error()
    assert lib.td_flux_set_controlnet_scales_at(f, -1, one, 1) == 2 and b"ControlNet -1 outside 0 .. 3" in lib.td_last_error()
    assert lib.td_flux_attached_controlnets(None, ctypes.byref(n)) == 2 and lib.td_flux_attached_controlnets(f, None) == 2 and n.value == -1
