"""FLUX ControlNet on the GPU: tiny models (oracle/flux_ref.tiny_config: D = 512; main model 2 double + 3 single blocks, 6 x 5 latent
tokens, T = 11) against the test-local reference tests/controlnet_common.py.  ControlNets: (n_d, n_s) = (1, 2) -- a repeated double
index and the single indices 0, 0, 1 --, (2, 0) -- no single injection -- and (2, 3) with num_mode = 2, mode 1.

Bars are the project's own (test_flux_kontext_gpu.py): against the bf16 reference rel-RMSE < 2e-2, against the fp32 reference
< 1.5 e_ref + 2e-3 with e_ref the bf16 reference's own distance from the fp32 one, measured here; int8 as test_int8_mode_on_a_conditioned_engine;
pixel RMSE < 1e-2.  What is an identity is held to bits."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import controlnet_common as C
from oracle import flux_ref as R
from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, preprocess_u8

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SCALING, SHIFT = 0.3611, 0.1159
S = C.H2 * C.W2
G35 = float((torch.tensor([3.5]).bfloat16() * 1000).float())


def _ops():
    from thinkdiff.ops import register
    return register()


def _i16(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_i16(a), _i16(b))


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _prepare(m, pe, pool, n, S_sched=S, ids=None, **kw):
    """set_condition + the n-step schedule of S_sched latent tokens; returns the sigmas."""
    from thinkdiff.models.flux_transformer import effective_scalar
    sig = R.make_sigmas(n, S_sched)
    m.set_condition(pe.cuda(), pool.cuda(), R.latent_image_ids(C.H2, C.W2) if ids is None else ids, **kw)
    m.set_timesteps([effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]], G35)
    return sig


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from kontext_common import build_engine
    cfg = C.main_config()
    sd = R.init_weights(cfg, seed=C.SEED_MAIN)
    lat, cond, cond2, pe, pool = C.inputs(cfg, S, C.T_TXT, C.SEED_IN)
    s = dict(cfg=cfg, sd=sd, tr=build_engine(cfg, sd), lat=lat, cond=cond, cond2=cond2, pe=pe, pool=pool, cn={})
    for name, (n_d, n_s, num_mode, mode) in C.CASES.items():
        cfg_cn = C.cn_config(n_d, n_s)
        sd_cn = C.cn_init_weights(cfg_cn, num_mode, seed=C.SEED_CN)
        s["cn"][name] = dict(cfg=cfg_cn, sd=sd_cn, model=C.build_controlnet(cfg_cn, sd_cn, num_mode), mode=mode)
    z = s["cn"]["1x2"]
    s["cn_zero"] = C.build_controlnet(z["cfg"], C.zero_outputs(z["sd"]))
    s["refs"] = {}
    return s


def _ref_args(s, dtype):
    """(lat, pe, pool, t, img_ids, txt_ids, guidance) of the one-step calls, in bf16 as the pipeline makes them or in fp32 for the yardstick."""
    t = torch.tensor([float(R.make_sigmas(2, S)[0]) * 1000.0]).bfloat16() / 1000
    ids = R.latent_image_ids(C.H2, C.W2)
    if dtype == BF:
        return s["lat"][None], s["pe"][None], s["pool"][None], t, ids.bfloat16(), torch.zeros(C.T_TXT, 3).bfloat16(), torch.tensor([3.5])
    return (s["lat"][None].float(), s["pe"][None].float(), s["pool"][None].float(), t.float(), ids, torch.zeros(C.T_TXT, 3),
            torch.tensor([G35 / 1000]))


def _refs(s, name):
    """The reference of one case, computed once: unscaled samples and the controlled forward at C.SCALE, bf16 and fp32, this and the other control."""
    if name in s["refs"]:
        return s["refs"][name]
    c = s["cn"][name]
    out = {}
    for tag, dtype in (("16", BF), ("32", torch.float32)):
        sd = {k: v.to(dtype) for k, v in s["sd"].items()}
        sd_cn = {k: v.to(dtype) for k, v in c["sd"].items()}
        x, e, p, t, ids, tids, g = _ref_args(s, dtype)
        bs, ss = C.controlnet_forward_ref(sd_cn, c["cfg"], x, s["cond"][None].to(dtype), c["mode"], e, p, t, ids, tids, None)
        out["samples" + tag] = torch.cat(bs + ss)
        out["v" + tag] = C.controlled_forward_ref(sd, s["cfg"], sd_cn, c["cfg"], x, s["cond"][None].to(dtype), c["mode"], e, p, t, ids, tids, g, C.SCALE)
    s["refs"][name] = out
    return out


def _prepare_pair(s, name, n=2, cond=None):
    """Main context and the case's ControlNet prepared for the same image, attached at the default scale 1.0."""
    c, m = s["cn"][name], s["tr"]
    sig = _prepare(m, s["pe"], s["pool"], n)
    cn = c["model"]
    _prepare(cn, s["pe"], s["pool"], n, control_mode=c["mode"])
    cn.set_control_condition((s["cond"] if cond is None else cond).cuda())
    m.attach_controlnet(cn)
    return m, cn, sig


# ---- 1. the inject kernel is bit-exact --------------------------------------------------------------------------------------------------
def _inject_data(rows, D, seed):
    """Magnitudes spread over 2^-8 .. 2^8 (an fma of product and sum rounds differently on such data), with +0 and -0 in both operands."""
    g = torch.Generator().manual_seed(seed)
    spread = lambda: torch.randn(rows, D, generator=g) * torch.exp2(torch.randint(-8, 9, (rows, D), generator=g).float())
    h, r = spread().bfloat16(), spread().bfloat16()
    h.view(-1)[0::7] = 0.0
    h.view(-1)[3::11] = -0.0
    r.view(-1)[1::5] = 0.0
    r.view(-1)[2::13] = -0.0
    return h, r


@pytest.mark.parametrize("scale", [1.0, 0.7, 0.35, 0.0])
@pytest.mark.parametrize("rows,D", [(1, 8), (37, 512), (30, 3072)])
def test_inject_bit_exact(hip, rows, D, scale):
    """flux_residual_inject_ against the eager statements on the device, bit for bit: (h.float() + (r.float() * s).bfloat16().float()).bfloat16();
    strided rows (ldh, ldr > D), columns beyond D untouched.  On the chosen data the fused form a + b * c differs (checked on the CPU)."""
    h, r = _inject_data(rows, D, rows * 31 + D)
    if scale in (0.7, 0.35) and rows > 1:
        s32 = torch.tensor(scale, dtype=torch.float32).double()
        unfused = (h.float() + (r.float() * scale).bfloat16().float()).bfloat16()
        fused = (h.double() + r.double() * s32).float().bfloat16()      # the product exact in fp64: one rounding, as an fma makes
        assert int((_i16(unfused) != _i16(fused)).sum()) > 0
    H = torch.full((rows, D + 24), 3.0, dtype=BF, device="cuda")
    Rr = torch.full((rows, D + 8), 5.0, dtype=BF, device="cuda")
    H[:, :D], Rr[:, :D] = h.cuda(), r.cuda()
    hv, rv = H[:, :D], Rr[:, :D]
    want = (hv.float() + (rv.float() * scale).bfloat16().float()).bfloat16()
    got = _ops().flux_residual_inject_(hv, rv, scale)
    torch.cuda.synchronize()
    assert got.data_ptr() == hv.data_ptr()
    assert _same(H[:, :D], want)
    assert bool((H[:, D:] == 3.0).all()) and bool((Rr[:, D:] == 5.0).all()) and _same(Rr[:, :D], r.cuda())
    if scale == 0.0:
        assert torch.equal(H[:, :D].float(), h.cuda().float())      # h + 0 is h (as values: -0 + 0 is +0)


def test_inject_refusals(hip):
    x = torch.zeros(16, 80, dtype=BF, device="cuda")
    inj = _ops().flux_residual_inject_
    with pytest.raises(RuntimeError, match="multiple of 8"):
        inj(x[:, :12], x[:, 16:28].clone(), 0.5)
    with pytest.raises(RuntimeError, match="16-byte"):
        inj(x[:, 4:36], x[:, 40:72].clone(), 0.5)
    with pytest.raises(RuntimeError, match="overlap"):
        inj(x[:, :32], x[:, 16:48], 0.5)
    with pytest.raises(RuntimeError, match="same row count"):
        inj(x[:, :32], x[:8, 40:72], 0.5)
    with pytest.raises(RuntimeError):
        inj(x[:, :32], x[:, 40:72].cpu(), 0.5)


# ---- 2. ControlNet samples ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_controlnet_samples_match_the_reference(setup, name):
    s, c = setup, setup["cn"][name]
    ref = _refs(s, name)
    cn = c["model"]
    _prepare(cn, s["pe"], s["pool"], 2, control_mode=c["mode"])
    cn.set_control_condition(s["cond"].cuda())
    bs, ss = cn.forward_samples(s["lat"].cuda(), 0)
    got = torch.cat(bs + ss).clone()
    cn.set_control_condition(s["cond2"].cuda())
    bs2, ss2 = cn.forward_samples(s["lat"].cuda(), 0)
    other = torch.cat(bs2 + ss2)
    torch.cuda.synchronize()
    n_d, n_s = c["cfg"].num_layers, c["cfg"].num_single_layers
    assert len(bs) == n_d and len(ss) == n_s and bs[0].shape == (S, c["cfg"].inner_dim)
    # the arena as td_flux_controlnet_samples describes it
    base, nd, ns, stride, rows, width = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    assert cn._L.td_flux_controlnet_samples(cn._h, *[ctypes.byref(v) for v in (base, nd, ns, stride, rows, width)]) == 0
    assert (nd.value, ns.value, rows.value, width.value) == (n_d, n_s, S, c["cfg"].inner_dim) and base.value and stride.value == cn.max_img_tokens * width.value
    # the text stream of a union model has one row more
    shp = [ctypes.c_int() for _ in range(4)]
    assert cn._L.td_flux_prepared_shape(cn._h, *[ctypes.byref(v) for v in shp]) == 0
    assert shp[1].value == C.T_TXT + (1 if c["mode"] is not None else 0)
    e16, e32 = C.rel_rmse(got, ref["samples16"].reshape(got.shape)), C.rel_rmse(got, ref["samples32"].reshape(got.shape))
    e_ref = C.rel_rmse(ref["samples16"], ref["samples32"])
    d_other = C.rel_rmse(other, got)
    print(f"{name}: samples hip~bf16-ref {e16:.4f}  hip~fp32-ref {e32:.4f}  bf16~fp32 ref {e_ref:.4f}  other control image {d_other:.3f}")
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3
    assert d_other > 0.1


def test_union_model_needs_a_mode(setup):
    c = setup["cn"]["2x3_union"]
    cn = c["model"]
    with pytest.raises(ValueError, match="control_mode is required"):
        cn.set_condition(setup["pe"].cuda(), setup["pool"].cuda(), R.latent_image_ids(C.H2, C.W2))
    L = cn._L
    assert L.td_flux_controlnet_set_mode(cn._h, -1) == 0
    pe, pool, ids = setup["pe"].cuda(), setup["pool"].cuda(), R.latent_image_ids(C.H2, C.W2).cuda()
    rc = L.td_flux_set_condition(cn._h, pe.data_ptr(), C.T_TXT, pool.data_ptr(), None, ids.data_ptr(), S, None)
    assert rc == 2 and b"union model (num_mode=2)" in L.td_last_error()
    assert L.td_flux_controlnet_set_mode(cn._h, 2) == 2 and b"mode 2 outside the 2 rows" in L.td_last_error()
    plain = setup["cn"]["1x2"]["model"]
    assert L.td_flux_controlnet_set_mode(plain._h, 0) == 2 and b"num_mode = 0" in L.td_last_error()
    torch.cuda.synchronize()


# ---- 3. the controlled forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_controlled_forward_matches_the_reference(setup, name):
    """Scale 0.7.  (1, 2): double index 0, 0 and single indices 0, 0, 1; (2, 0): no single injection.  The text rows are never injected: the
    reference adds single samples to the image rows only, at T = 11 with non-zero samples, and the engine agrees with it."""
    s = setup
    ref = _refs(s, name)
    m, cn, _ = _prepare_pair(s, name)
    try:
        m.set_controlnet_scales([C.SCALE, C.SCALE])
        v = m.forward_step(s["lat"].cuda(), 0).clone()
        cn.set_control_condition(s["cond2"].cuda())
        v_other = m.forward_step(s["lat"].cuda(), 0).clone()
    finally:
        m.attach_controlnet(None)
    v_plain = m.forward_step(s["lat"].cuda(), 0)
    torch.cuda.synchronize()
    e16, e32, e_ref = C.rel_rmse(v[None], ref["v16"]), C.rel_rmse(v[None], ref["v32"]), C.rel_rmse(ref["v16"], ref["v32"])
    d_other, d_plain = C.rel_rmse(v_other, v), C.rel_rmse(v_plain, v)
    print(f"{name}: controlled forward hip~bf16-ref {e16:.4f}  hip~fp32-ref {e32:.4f}  bf16~fp32 ref {e_ref:.4f};  moved by: other control "
          f"{d_other:.3f}  no ControlNet {d_plain:.3f}")
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3
    assert d_other > 0.1 and d_plain > 0.1


# ---- 4. parent identity -------------------------------------------------------------------------------------------------------------------
def test_parent_identity(setup):
    """Bit-equal to the unattached forward: attached with scale 0 at the step; attached at scale 1 with all-zero output Linears; after detaching."""
    s, m = setup, setup["tr"]
    lat = s["lat"].cuda()
    _prepare(m, s["pe"], s["pool"], 2)
    v0 = [m.forward_step(lat, i).clone() for i in range(2)]
    m, cn, _ = _prepare_pair(s, "1x2")
    try:
        v_on = m.forward_step(lat, 0).clone()
        m.set_controlnet_scales([0.0, 1.0])
        v_s0 = m.forward_step(lat, 0).clone()
        v_s1 = m.forward_step(lat, 1).clone()
        m.set_controlnet_scales([0.0, 0.0])
        v_z = [m.forward_step(lat, i).clone() for i in range(2)]
        zero = s["cn_zero"]
        _prepare(zero, s["pe"], s["pool"], 2)
        zero.set_control_condition(s["cond"].cuda())
        m.attach_controlnet(zero)                 # (attaching resets the scales to 1.0)
        v_zero = m.forward_step(lat, 0).clone()
    finally:
        m.attach_controlnet(None)
    v_off = m.forward_step(lat, 0).clone()
    torch.cuda.synchronize()
    assert not _same(v_on, v0[0]) and not _same(v_s1, v0[1])
    assert _same(v_s0, v0[0]) and _same(v_z[0], v0[0]) and _same(v_z[1], v0[1])
    assert _same(v_zero, v0[0])
    assert _same(v_off, v0[0])


# ---- 5. the denoise loop ------------------------------------------------------------------------------------------------------------------
def test_denoise_loop_single_and_in_flight(setup):
    """4 steps, scales [0.7, 0.7, 0, 0]: td_flux_denoise, and td_flux_denoise_multi with two main contexts, two ControlNet forks and two control
    images; each against the reference loop, and each image in flight bit-equal to its single-image run."""
    s, name, n = setup, "1x2", 4
    c = s["cn"][name]
    scales = [C.SCALE, C.SCALE, 0.0, 0.0]
    refs = [C.denoise_ref(s["sd"], s["cfg"], c["sd"], c["cfg"], s["lat"][None], cd[None], c["mode"], s["pe"][None], s["pool"][None], C.H2, C.W2, n, scales)
            for cd in (s["cond"], s["cond2"])]
    singles = []
    for cd in (s["cond"], s["cond2"]):
        m, cn, sig = _prepare_pair(s, name, n, cond=cd)
        try:
            m.set_controlnet_scales(scales)
            x = s["lat"].cuda().clone()
            m.denoise(x, sig)
            singles.append(x)
        finally:
            m.attach_controlnet(None)
    m2, cn2 = s["tr"].fork(), c["model"].fork()
    ctxs, cns = [s["tr"], m2], [c["model"], cn2]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    xs = [s["lat"].cuda().clone() for _ in range(2)]
    torch.cuda.synchronize()
    try:
        for k, cd in enumerate((s["cond"], s["cond2"])):
            sig = _prepare(ctxs[k], s["pe"], s["pool"], n)
            _prepare(cns[k], s["pe"], s["pool"], n, control_mode=c["mode"])
            cns[k].set_control_condition(cd.cuda())
            ctxs[k].attach_controlnet(cns[k])
            ctxs[k].set_controlnet_scales(scales)
        # one ControlNet context serves one main context at a time
        with pytest.raises(Exception, match="already serves another main context"):
            m2.attach_controlnet(c["model"])
        torch.cuda.synchronize()
        type(s["tr"]).denoise_multi(ctxs, xs, sig, streams)
        torch.cuda.synchronize()
    finally:
        for ctx in ctxs:
            ctx.attach_controlnet(None)
    for k in range(2):
        e = C.rel_rmse(singles[k][None], refs[k])
        print(f"image {k}: denoise hip~bf16-ref {e:.4f}; in flight == single: {_same(xs[k], singles[k])}")
        assert e < 2e-2
        assert _same(xs[k], singles[k])
    assert C.rel_rmse(singles[1], singles[0]) > 0.05


# ---- 6. refusals on the engine ------------------------------------------------------------------------------------------------------------
def _refused(m, lat, *words):
    L = m._L
    out = torch.empty_like(lat)
    rc = L.td_flux_forward(m._h, lat.data_ptr(), 0, out.data_ptr(), None)
    msg = L.td_last_error()
    assert rc == 2 and all(w.encode() in msg for w in words), (rc, msg)


def test_engine_refusals(setup):
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig
    s, m = setup, setup["tr"]
    lat = s["lat"].cuda()
    L = m._L
    torch.cuda.synchronize()
    try:
        # another inner width / head count
        cfg8 = R.tiny_config(num_layers=1, num_single_layers=0, num_attention_heads=8, guidance_embeds=False)
        wide = C.build_controlnet(cfg8, C.cn_init_weights(cfg8, 0, seed=1))
        _prepare(m, s["pe"], s["pool"], 2)
        _prepare(wide, s["pe"], s["pool"], 2)
        m.attach_controlnet(wide)
        _refused(m, lat, "inner width 1024 (8 heads)", "512 (4 heads)")
        # another latent width
        cfg128 = R.tiny_config(num_layers=1, num_single_layers=0, in_channels=128, guidance_embeds=False)
        fat = C.build_controlnet(cfg128, C.cn_init_weights(cfg128, 0, seed=2))
        _prepare(fat, s["pe"], s["pool"], 2)
        m.attach_controlnet(fat)
        _refused(m, lat, "reads 128 latent channels", "steps 64")
        # the case's own ControlNet: no control condition; another S_img; another step count
        cn = s["cn"]["1x2"]["model"]
        _prepare(cn, s["pe"], s["pool"], 2, ids=R.latent_image_ids(4, 4))      # (another S_img voids the control condition)
        m.attach_controlnet(cn)
        _refused(m, lat, "prepared for 16 image tokens", f"for {S}")
        _prepare(cn, s["pe"], s["pool"], 2)
        _refused(m, lat, "no control condition", f"{S} image tokens")
        cn.set_control_condition(s["cond"].cuda())
        _prepare(cn, s["pe"], s["pool"], 3)
        cn.set_control_condition(s["cond"].cuda())
        _refused(m, lat, "prepared for 3 timesteps", "for 2")
        _prepare(cn, s["pe"], s["pool"], 2)
        cn.set_control_condition(s["cond"].cuda())
        # reference tokens on the main context
        from kontext_common import reference_ids
        m.set_reference_tokens(torch.zeros(4, C.LAT, dtype=BF, device="cuda"), reference_ids(2, 2))
        _refused(m, lat, "4 reference tokens")
        m.set_reference_tokens(None)
        m.forward_step(lat, 0)                      # ... and with everything in place it runs
        # td_flux_forward on a ControlNet context; precision and LoRA on a ControlNet model
        out = torch.empty_like(lat)
        assert L.td_flux_forward(cn._h, lat.data_ptr(), 0, out.data_ptr(), None) == 2 and b"ControlNet context has no velocity" in L.td_last_error()
        assert L.td_flux_set_precision(cn._h, 2, None) == 2 and b"precision 2 on a ControlNet model" in L.td_last_error()
        assert L.td_flux_set_attention(cn._h, 1) == 2 and b"ControlNet model" in L.td_last_error()
        A = torch.zeros(4, 64, dtype=BF, device="cuda")
        B = torch.zeros(512, 4, dtype=BF, device="cuda")
        assert L.td_flux_lora_load(cn._h, b"a", b"x_embedder.weight", A.data_ptr(), B.data_ptr(), 4, 1.0, None) == 2
        assert b"'x_embedder.weight' on a ControlNet model" in L.td_last_error()
        assert L.td_flux_set_reference_tokens(cn._h, A.data_ptr(), 1, A.data_ptr(), None) == 2 and b"ControlNet context" in L.td_last_error()
        # attachments of the wrong kind, and scales without an attachment
        assert L.td_flux_attach_controlnet(cn._h, cn._h) == 2 and b"first argument is a ControlNet context" in L.td_last_error()
        assert L.td_flux_attach_controlnet(m._h, m._h) == 2 and b"not a ControlNet context" in L.td_last_error()
        assert L.td_flux_controlnet_forward(m._h, lat.data_ptr(), 0, None) == 2 and b"not a ControlNet context" in L.td_last_error()
        m.attach_controlnet(None)
        one = (ctypes.c_float * 1)(1.0)
        assert L.td_flux_set_controlnet_scales(m._h, ctypes.cast(one, ctypes.c_void_p), 1) == 2 and b"no ControlNet is attached" in L.td_last_error()
        # a channel-conditioned main engine
        cc = FluxTransformer2DModel(FluxTransformerConfig(in_channels=128, out_channels=64, num_layers=1, num_single_layers=1, num_attention_heads=4,
                                                          joint_attention_dim=s["cfg"].joint_attention_dim, pooled_projection_dim=s["cfg"].pooled_projection_dim),
                                    max_img_tokens=64, max_txt_tokens=32, max_steps=4).init_random(3)
        _prepare(cc, s["pe"], s["pool"], 2)
        cc.set_channel_condition(torch.zeros(S, 64, dtype=BF, device="cuda"))
        cc.attach_controlnet(cn)
        _refused(cc, lat, "channel-conditioned transformer (in_channels=128, out_channels=64)")
        cc.attach_controlnet(None)
    finally:
        m.attach_controlnet(None)
        torch.cuda.synchronize()


# ---- 7. an 8-bit main model with a bf16 ControlNet ------------------------------------------------------------------------------------------
def test_int8_main_model_with_a_bf16_controlnet(setup):
    """int8 with dynamic scales on the main transformer, the side network in bf16: finite; against the int8-configured reference under
    test_int8_mode_on_a_conditioned_engine's bars; back in bf16 the bf16 bits return."""
    s, name = setup, "1x2"
    c = s["cn"][name]
    x, e, p, t, ids, tids, g = _ref_args(s, BF)
    args = (s["sd"], s["cfg"], c["sd"], c["cfg"], x, s["cond"][None], c["mode"], e, p, t, ids, tids, g, C.SCALE)
    ref16 = _refs(s, name)["v16"]
    R.INT8_BLOCK_LINEARS = True
    try:
        ref8 = C.controlled_forward_ref(*args)
    finally:
        R.INT8_BLOCK_LINEARS = False
    m, cn, _ = _prepare_pair(s, name)
    lat = s["lat"].cuda()
    try:
        m.set_controlnet_scales([C.SCALE, C.SCALE])
        out16 = m.forward_step(lat, 0).clone()
        try:
            m.set_precision("int8")
            out8 = m.forward_step(lat, 0).clone()
        finally:
            m.set_precision("bf16")
        back = m.forward_step(lat, 0).clone()
    finally:
        m.attach_controlnet(None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out8.float()).all())
    e16, e88, d_hip, d_ref = C.rel_rmse(out16[None], ref16), C.rel_rmse(out8[None], ref8), C.rel_rmse(out8, out16), C.rel_rmse(ref8, ref16)
    print(f"int8 main + bf16 ControlNet: hip~bf16-ref {e16:.4f}  hip-int8~ref-int8 {e88:.4f}  int8~bf16 hip {d_hip:.4f} ref {d_ref:.4f}")
    assert e16 < 2e-2 and e88 < 2e-2
    assert d_hip < 3e-2 and abs(d_hip - d_ref) < 0.5 * d_ref + 2e-3
    assert _same(back, out16)


# ---- 8. the pipeline ----------------------------------------------------------------------------------------------------------------------
def _image(n, seed):
    from PIL import Image
    u8 = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    u8 = F.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return Image.fromarray(u8.numpy()), u8


@pytest.fixture(scope="module")
def pipe(setup):
    from thinkdiff.models import FluxControlNetPipelineRewritePrompt, FluxPipelineRewritePrompt
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder, AutoencoderKLEncoder
    s = setup
    vcfg = V.VaeConfig()
    sd_dec, sd_enc = V.init_weights(vcfg, seed=12), encoder_init_weights(vcfg, seed=13)
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(16, 16))
    dec.load_state_dict(sd_dec)
    enc = AutoencoderKLEncoder(AutoencoderKLConfig(), max_image_size=(128, 128))
    enc.load_state_dict(sd_enc)
    c = s["cn"]["1x2"]
    g = torch.Generator().manual_seed(21)
    return dict(vcfg=vcfg, sd_dec=sd_dec, sd_enc=sd_enc, c=c,
                pipe=FluxControlNetPipelineRewritePrompt(transformer=s["tr"], vae=dec, vae_encoder=enc, controlnet=c["model"]),
                t2i=FluxPipelineRewritePrompt(transformer=s["tr"], vae=dec),
                pe=torch.randn(1, 24, s["cfg"].joint_attention_dim, generator=g).bfloat16().cuda(),
                pool=torch.randn(1, s["cfg"].pooled_projection_dim, generator=g).bfloat16().cuda())


def _kw(p, **more):
    return dict(prompt_embeds=p["pe"], pooled_prompt_embeds=p["pool"], height=128, width=128, num_inference_steps=3, guidance_scale=3.5, **more)


def test_pipeline_matches_the_cpu_loop(setup, pipe):
    """128 x 128, 3 steps, scale 0.7, control_guidance_end 0.7 (keep 1, 1, 0): eps for the control image first, then the noise."""
    s, p, N = setup, pipe, 3
    img, u8 = _image(128, 3)
    kw = _kw(p, control_image=img, controlnet_conditioning_scale=C.SCALE, control_guidance_end=0.7)
    out = p["pipe"](generator=_gen(8), output_type="latent", **kw).images
    px = p["pipe"](generator=_gen(8), output_type="np", **kw).images
    g = _gen(8)
    eps = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    mom = encode_ref(p["sd_enc"], p["vcfg"], preprocess_u8(u8))
    cond = latents_ref(mom, eps, None, 0.0, SCALING, SHIFT)
    scales = [C.SCALE * k for k in C.keep_schedule(N, 0.0, 0.7)]
    assert scales == [C.SCALE, C.SCALE, 0.0]
    c = p["c"]
    x = C.denoise_ref(s["sd"], s["cfg"], c["sd"], c["cfg"], R.pack_latents(noise), cond, c["mode"], p["pe"].cpu(), p["pool"].cpu(), 8, 8, N, scales)
    _, ref_u8 = V.latents_to_image(p["sd_dec"], p["vcfg"], x, 16, 16)
    rel = C.rel_rmse(out[0], x[0])
    prmse = float(((px[0].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"controlnet pipeline 128x128, {N} steps: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}")
    assert rel < 2e-2 and prmse < 1e-2


@pytest.mark.parametrize("case", ["default", "latents", "control_image_as_latents"])
def test_pipeline_generator_position_after_a_call(pipe, case):
    """eps [B_img] (not with a latent control_image) first, then noise [B] (not with latents=)."""
    img, _ = _image(128, 9)
    shape = (1, 16, 16, 16)
    g, r = _gen(13), _gen(13)
    kw, draws = _kw(pipe, control_image=img, output_type="latent"), 2
    if case == "latents":
        kw["latents"], draws = torch.zeros(1, 64, C.LAT, dtype=BF, device="cuda"), 1
    elif case == "control_image_as_latents":
        kw["control_image"], draws = torch.zeros(1, 16, 16, 16, dtype=BF, device="cuda"), 1
    pipe["pipe"](generator=g, **kw)
    after = torch.randn(64, generator=g, device="cuda", dtype=BF)
    for _ in range(draws):
        torch.randn(shape, generator=r, device="cuda", dtype=BF)
    want = torch.randn(64, generator=r, device="cuda", dtype=BF)
    assert torch.equal(_i16(after), _i16(want))


def test_pipeline_guidance_end_zero_is_the_plain_pipeline_and_latent_control_is_used_as_it_is(setup, pipe):
    s, p = setup, pipe
    img, _ = _image(128, 5)
    lat0 = torch.randn(1, 64, C.LAT, generator=_gen(2), device="cuda", dtype=BF)
    kw = _kw(p, output_type="latent", latents=lat0)
    plain = p["t2i"](**kw).images
    off = p["pipe"](control_image=img, control_guidance_end=0.0, **kw).images
    on = p["pipe"](control_image=img, **kw).images
    assert _same(off, plain) and not _same(on, plain)
    # a latent-shaped control image: packed as it is -- the engine run on flux_pack_latents(z) gives the same bits
    z = torch.randn(1, 16, 16, 16, generator=_gen(4), device="cuda", dtype=BF)
    got = p["pipe"](control_image=z, controlnet_conditioning_scale=C.SCALE, **kw).images
    from thinkdiff.models.flux_transformer import effective_scalar
    m, cn = s["tr"], p["c"]["model"]
    sig = R.make_sigmas(3, 64)
    t_eff = [effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]]
    ids = R.latent_image_ids(8, 8)
    try:
        m.set_condition(p["pe"][0], p["pool"][0], ids)
        m.set_timesteps(t_eff, G35)
        cn.set_condition(p["pe"][0], p["pool"][0], ids, control_mode=p["c"]["mode"])
        cn.set_control_condition(_ops().flux_pack_latents(z[0].contiguous()))
        cn.set_timesteps(t_eff, 0.0)
        m.attach_controlnet(cn)
        m.set_controlnet_scales([C.SCALE] * 3)
        x = lat0[0].clone()
        m.denoise(x, sig)
    finally:
        m.attach_controlnet(None)
    torch.cuda.synchronize()
    assert _same(got[0], x)
    assert _same(lat0, torch.randn(1, 64, C.LAT, generator=_gen(2), device="cuda", dtype=BF))      # the caller's latents are not mutated


def test_pipeline_images_in_flight_and_control_per_context(pipe):
    """Two images of one call with two control images: advanced two in flight (one transformer fork + one ControlNet fork per image) they
    are bit-identical to one at a time, each image follows ITS control image, and the transformer's contexts are left plain."""
    p = pipe["pipe"]
    z = torch.randn(2, 16, 16, 16, generator=_gen(6), device="cuda", dtype=BF)
    lat0 = torch.randn(2, 64, C.LAT, generator=_gen(7), device="cuda", dtype=BF)
    kw = _kw(pipe, output_type="latent", latents=lat0, control_image=z, controlnet_conditioning_scale=C.SCALE, num_images_per_prompt=2)
    old = p.images_in_flight
    try:
        p.images_in_flight = 2
        two = p(**kw).images
        p.images_in_flight = 1
        one = p(**kw).images
        swapped = p(**{**kw, "control_image": z.flip(0).contiguous()}).images
    finally:
        p.images_in_flight = old
    assert two.shape == (2, 64, C.LAT) and _same(two, one)
    assert not _same(two[0], two[1]) and not _same(swapped[0], one[0])
    same_lat = _kw(pipe, output_type="latent", latents=lat0[:1])
    assert _same(p(control_image=z[1:], controlnet_conditioning_scale=C.SCALE, **same_lat).images[0], swapped[0])      # image 0 under control image 1
    plain = pipe["t2i"](**same_lat).images
    assert _same(p(control_image=z[:1], control_guidance_end=0.0, **same_lat).images, plain)
