"""Several FLUX ControlNets on one transformer, on the GPU: the tiny models of tests/controlnet_common.py (main model 2 double + 3 single
blocks, 6 x 5 latent tokens, T = 11) against the test-local reference tests/multi_controlnet_common.py.  The two nets: case "1x2" on
`cond` at 0.7 and case "2x3_union" at mode 1 on `cond2` at 0.45 -- sample counts (1, 2) against (2, 3), so every net's own index rule is
exercised behind both kinds of block.

Bars are the project's own (test_flux_controlnet_gpu.py): against the bf16 reference rel-RMSE < 2e-2, against the fp32 reference
< 1.5 e_ref + 2e-3 with e_ref the bf16 reference's own distance from the fp32 one, measured here.  What is an identity is held to bits."""
import ctypes

import pytest
import torch

import controlnet_common as C
import multi_controlnet_common as M
from oracle import flux_ref as R
from oracle import vae_ref as V

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
S = C.H2 * C.W2
G35 = float((torch.tensor([3.5]).bfloat16() * 1000).float())
SC0, SC1 = M.NETS[0][2], M.NETS[1][2]


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
    s = dict(cfg=cfg, sd=sd, tr=build_engine(cfg, sd), lat=lat, cond=cond, cond2=cond2, pe=pe, pool=pool, cn=[])
    for (case, _, _), seed in zip(M.NETS, (C.SEED_CN, M.SEED_CN2)):
        n_d, n_s, num_mode, mode = C.CASES[case]
        cfg_cn = C.cn_config(n_d, n_s)
        sd_cn = C.cn_init_weights(cfg_cn, num_mode, seed=seed)
        s["cn"].append(dict(cfg=cfg_cn, sd=sd_cn, num_mode=num_mode, model=C.build_controlnet(cfg_cn, sd_cn, num_mode), mode=mode))
    return s


def _attach(s, m, entries, n=2, tables=None):
    """Main context `m` and the listed (ControlNet context, mode, control latents) prepared for the same image and attached in that
    order; tables: per-net scale tables (None: the 1.0 attaching leaves)."""
    sig = _prepare(m, s["pe"], s["pool"], n)
    for cn, mode, cond in entries:
        _prepare(cn, s["pe"], s["pool"], n, control_mode=mode)
        cn.set_control_condition(cond.cuda())
    m.attach_controlnets([e[0] for e in entries])
    for k, t in enumerate(tables or []):
        m.set_controlnet_scales(t, net=k)
    return sig


def _two(s, conds=("cond", "cond2"), models=None):
    models = models or [c["model"] for c in s["cn"]]
    return [(models[k], s["cn"][k]["mode"], s[conds[k]]) for k in range(2)]


# ---- 1. the kernel, bit for bit -------------------------------------------------------------------------------------------------------------
SCALES = [0.7, 0.45, 1.0, 3.7]


def _spread(rows, cols, g):
    """Magnitudes spread over 2^-8 .. 2^8 (a contracted product-and-sum rounds differently on such data), with +0 and -0 sprinkled in."""
    x = torch.randn(rows, cols, generator=g, device="cuda") * torch.exp2(torch.randint(-8, 9, (rows, cols), generator=g, device="cuda").float())
    x = x.bfloat16()
    x.view(-1)[0::7] = 0.0
    x.view(-1)[3::11] = -0.0
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("rows,D,ldh,ldr1", [(1, 8, 32, 8), (3, 72, 80, 96), (257, 3072, 3080, 3072), (4096, 3072, 3080, 3072)])
def test_inject_multi_bit_exact(hip, rows, D, ldh, ldr1, n):
    """flux_residual_inject_multi_ against the eager statements on the device, bit for bit:
        acc = bf16(s_0 * r_0);  acc = bf16(acc + bf16(s_k * r_k)) for k = 1 .. n-1;  h = bf16(h + acc)
    with strided h (ldh > D) and, from the second operand on, one strided r (ldr1); columns of h beyond D untouched; n = 1 equals
    flux_residual_inject_; n >= 2 differs from n successive single injections on the two large shapes (which is why the sum is its own kernel)."""
    g = _gen(rows * 31 + D + n)
    H = torch.full((rows, ldh), 3.0, dtype=BF, device="cuda")
    H[:, :D] = _spread(rows, D, g)
    h0 = H[:, :D].clone()
    rs = []
    for k in range(n):
        ld = ldr1 if k == 1 else D
        Rk = torch.full((rows, ld), 5.0, dtype=BF, device="cuda")
        Rk[:, :D] = _spread(rows, D, g)
        rs.append(Rk[:, :D])
    sc = SCALES[:n]
    acc = (rs[0].float() * sc[0]).bfloat16()
    for k in range(1, n):
        acc = (acc.float() + (rs[k].float() * sc[k]).bfloat16().float()).bfloat16()
    want = (h0.float() + acc.float()).bfloat16()
    keep = [r.clone() for r in rs]
    hv = H[:, :D]
    got = _ops().flux_residual_inject_multi_(hv, rs, sc)
    torch.cuda.synchronize()
    assert got.data_ptr() == hv.data_ptr()
    assert _same(H[:, :D], want)
    assert bool((H[:, D:] == 3.0).all()) and all(_same(a, b) for a, b in zip(rs, keep))
    one_by_one = h0.clone()
    for k in range(n):
        _ops().flux_residual_inject_(one_by_one, rs[k], sc[k])
    torch.cuda.synchronize()
    if n == 1:
        assert _same(one_by_one, want)
    elif rows >= 257:
        assert int((_i16(one_by_one) != _i16(want)).sum()) > 0


def test_inject_multi_refusals(hip):
    x = torch.zeros(16, 160, dtype=BF, device="cuda")
    inj = _ops().flux_residual_inject_multi_
    a, b = x[:, 40:72].clone(), x[:, 80:112].clone()
    with pytest.raises(RuntimeError, match="as many scales"):
        inj(x[:, :32], [a, b], [0.5])
    with pytest.raises(RuntimeError, match="1 .. 4 tensors"):
        inj(x[:, :32], [a] * 5, [0.5] * 5)
    with pytest.raises(RuntimeError, match="1 .. 4 tensors"):
        inj(x[:, :32], [], [])
    with pytest.raises(RuntimeError, match="same row count and width"):
        inj(x[:, :32], [a, b[:, :24]], [0.5, 0.5])
    with pytest.raises(RuntimeError, match=r"r\[1\] must be 16-byte aligned"):
        inj(x[:, :32], [a, x[:, 44:76]], [0.5, 0.5])
    with pytest.raises(RuntimeError, match=r"r\[1\] must not overlap h"):
        inj(x[:, :32], [a, x[:, 16:48]], [0.5, 0.5])
    with pytest.raises(RuntimeError, match="multiple of 8"):
        inj(x[:, :12], [x[:, 16:28].clone(), x[:, 32:44].clone()], [0.5, 0.5])
    with pytest.raises(RuntimeError, match=r"scales\[1\] is not finite"):
        inj(x[:, :32], [a, b], [0.5, float("inf")])
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# ---- 2. one forward with two different nets -------------------------------------------------------------------------------------------------
def _ref_args(s, dtype):
    t = torch.tensor([float(R.make_sigmas(2, S)[0]) * 1000.0]).bfloat16() / 1000
    ids = R.latent_image_ids(C.H2, C.W2)
    if dtype == BF:
        return s["lat"][None], s["pe"][None], s["pool"][None], t, ids.bfloat16(), torch.zeros(C.T_TXT, 3).bfloat16(), torch.tensor([3.5])
    return (s["lat"][None].float(), s["pe"][None].float(), s["pool"][None].float(), t.float(), ids, torch.zeros(C.T_TXT, 3),
            torch.tensor([G35 / 1000]))


def _ref(s, dtype, conds=("cond", "cond2"), scales=(SC0, SC1)):
    sd = {k: v.to(dtype) for k, v in s["sd"].items()}
    nets = [M.net({k: v.to(dtype) for k, v in c["sd"].items()}, c["cfg"], s[cd][None].to(dtype), c["mode"], sc)
            for c, cd, sc in zip(s["cn"], conds, scales)]
    x, e, p, t, ids, tids, g = _ref_args(s, dtype)
    return M.multi_controlled_forward_ref(sd, s["cfg"], nets, x, e, p, t, ids, tids, g)


def test_forward_with_two_nets_matches_the_reference(setup):
    """Measured on the CPU for these seeds and scales (reference alone): e_ref 0.007, drop net 1 0.156, drop net 0 0.326, swap the control
    images 0.343, no nets 0.357."""
    s, m = setup, setup["tr"]
    v16, v32 = _ref(s, BF), _ref(s, torch.float32)
    e_ref = C.rel_rmse(v16, v32)
    d_ref = dict(drop1=C.rel_rmse(_ref(s, BF, scales=(SC0, 0.0)), v16), drop0=C.rel_rmse(_ref(s, BF, scales=(0.0, SC1)), v16),
                 swap=C.rel_rmse(_ref(s, BF, conds=("cond2", "cond")), v16))
    print(f"reference: e_ref {e_ref:.4f}  " + "  ".join(f"{k} {v:.3f}" for k, v in d_ref.items()))
    assert all(v > 0.05 for v in d_ref.values())      # the reference alone, before the engine is judged
    lat = s["lat"].cuda()
    try:
        _attach(s, m, _two(s), tables=[[SC0] * 2, [SC1] * 2])
        assert m.attached_controlnets() == 2
        v = m.forward_step(lat, 0).clone()
        m.set_controlnet_scales([0.0, 0.0], net=1)
        v_drop1 = m.forward_step(lat, 0).clone()
        m.set_controlnet_scales([SC1] * 2, net=1)
        m.set_controlnet_scales([0.0, 0.0], net=0)
        v_drop0 = m.forward_step(lat, 0).clone()
        _attach(s, m, _two(s, conds=("cond2", "cond")), tables=[[SC0] * 2, [SC1] * 2])
        v_swap = m.forward_step(lat, 0).clone()
    finally:
        m.attach_controlnets([])
    torch.cuda.synchronize()
    e16, e32 = C.rel_rmse(v[None], v16), C.rel_rmse(v[None], v32)
    d = dict(drop1=C.rel_rmse(v_drop1, v), drop0=C.rel_rmse(v_drop0, v), swap=C.rel_rmse(v_swap, v))
    print(f"two nets: hip~bf16-ref {e16:.4f}  hip~fp32-ref {e32:.4f}  bf16~fp32 ref {e_ref:.4f};  moved by: " + "  ".join(f"{k} {x:.3f}" for k, x in d.items()))
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3
    assert all(x > 0.05 for x in d.values())


# ---- 3. identities, held to bits ------------------------------------------------------------------------------------------------------------
def test_identities(setup):
    s, m = setup, setup["tr"]
    lat = s["lat"].cuda()
    a, b = _two(s)
    _prepare(m, s["pe"], s["pool"], 2)
    plain = [m.forward_step(lat, i).clone() for i in range(2)]
    try:
        # the list API with K = 1 is td_flux_attach_controlnet
        _attach(s, m, [a], tables=[[SC0] * 2])
        one_list = m.forward_step(lat, 0).clone()
        m.attach_controlnet(a[0])
        assert m.attached_controlnets() == 1
        m.set_controlnet_scales([SC0] * 2)
        one_old = m.forward_step(lat, 0).clone()
        # K = 2 with net 1's table all zero is net 0 alone; with net 0's all zero, net 1 alone
        _attach(s, m, [a, b], tables=[[SC0] * 2, [0.0, 0.0]])
        two_off1 = m.forward_step(lat, 0).clone()
        _attach(s, m, [b], tables=[[SC1] * 2])
        only_b = m.forward_step(lat, 0).clone()
        _attach(s, m, [a, b], tables=[[0.0, 0.0], [SC1] * 2])
        two_off0 = m.forward_step(lat, 0).clone()
        # all tables zero, and n = 0, are the plain context
        m.set_controlnet_scales([0.0, 0.0], net=1)
        all_zero = [m.forward_step(lat, i).clone() for i in range(2)]
        m.attach_controlnets([])
        assert m.attached_controlnets() == 0
        detached = m.forward_step(lat, 0).clone()
        # attaching resets every table to 1.0
        _attach(s, m, [a, b], tables=[[0.0, 0.0], [0.0, 0.0]])
        m.attach_controlnets([a[0], b[0]])
        reset = m.forward_step(lat, 0).clone()
        _attach(s, m, [a, b], tables=[[1.0, 1.0], [1.0, 1.0]])
        ones = m.forward_step(lat, 0).clone()
    finally:
        m.attach_controlnets([])
    torch.cuda.synchronize()
    assert _same(one_list, one_old) and not _same(one_list, plain[0])
    assert _same(two_off1, one_list)
    assert _same(two_off0, only_b) and not _same(only_b, one_list)
    assert _same(all_zero[0], plain[0]) and _same(all_zero[1], plain[1]) and _same(detached, plain[0])
    assert _same(reset, ones) and not _same(reset, plain[0])


def test_one_union_model_listed_twice_equals_two_loaded_copies(setup):
    """Two forks of ONE union model under modes 0 and 1 with two control images, against two separately loaded copies of it."""
    s, m = setup, setup["tr"]
    lat = s["lat"].cuda()
    u = s["cn"][1]
    copy = C.build_controlnet(u["cfg"], u["sd"], u["num_mode"])
    fork = u["model"].fork()
    tables = [[SC0] * 2, [SC1] * 2]
    try:
        _attach(s, m, [(u["model"], 0, s["cond"]), (fork, 1, s["cond2"])], tables=tables)
        twice = m.forward_step(lat, 0).clone()
        _attach(s, m, [(u["model"], 0, s["cond"]), (copy, 1, s["cond2"])], tables=tables)
        copies = m.forward_step(lat, 0).clone()
        _attach(s, m, [(u["model"], 0, s["cond"])], tables=tables[:1])
        first = m.forward_step(lat, 0).clone()
        # the same CONTEXT twice is refused, and nothing changes
        L = m._L
        arr = (ctypes.c_void_p * 2)(fork._h.value, fork._h.value)
        assert L.td_flux_attach_controlnets(m._h, ctypes.cast(arr, ctypes.c_void_p), 2) == 2 and b"same ControlNet context" in L.td_last_error()
        assert m.attached_controlnets() == 1
    finally:
        m.attach_controlnets([])
    torch.cuda.synchronize()
    assert _same(twice, copies) and not _same(twice, first)


# ---- 4. the denoise loop --------------------------------------------------------------------------------------------------------------------
TABLES = [[SC0, SC0, 0.0, 0.0, SC0], [0.0, SC1, 0.0, SC1, SC1]]      # only net 0, both, neither, only net 1, both


def test_denoise_loop_single_and_in_flight(setup):
    """5 steps: td_flux_denoise against the reference loop, and td_flux_denoise_multi with two main contexts x two ControlNet forks, image 1
    with the control images the other way round: bit-equal to one at a time, each image following ITS control images."""
    s, n = setup, 5
    orders = (("cond", "cond2"), ("cond2", "cond"))
    nets = lambda conds: [M.net(c["sd"], c["cfg"], s[cd][None], c["mode"], None) for c, cd in zip(s["cn"], conds)]
    ref = M.multi_denoise_ref(s["sd"], s["cfg"], nets(orders[0]), s["lat"][None], s["pe"][None], s["pool"][None], C.H2, C.W2, n, TABLES)
    m = s["tr"]
    singles = []
    for conds in orders:
        try:
            sig = _attach(s, m, _two(s, conds), n, TABLES)
            x = s["lat"].cuda().clone()
            m.denoise(x, sig)
            singles.append(x)
        finally:
            m.attach_controlnets([])
    m2 = m.fork()
    forks = [c["model"].fork() for c in s["cn"]]
    ctxs = [m, m2]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    xs = [s["lat"].cuda().clone() for _ in range(2)]
    torch.cuda.synchronize()
    try:
        sig = _attach(s, m, _two(s, orders[0]), n, TABLES)
        _attach(s, m2, _two(s, orders[1], models=forks), n, TABLES)
        # one ControlNet context serves one main context at a time, under the list form too
        with pytest.raises(Exception, match="already serves another main context"):
            m2.attach_controlnets([forks[0], s["cn"][1]["model"]])
        assert m2.attached_controlnets() == 2
        torch.cuda.synchronize()
        type(m).denoise_multi(ctxs, xs, sig, streams)
        torch.cuda.synchronize()
    finally:
        for ctx in ctxs:
            ctx.attach_controlnets([])
    e = C.rel_rmse(singles[0][None], ref)
    print(f"denoise, 5 steps, two nets: hip~bf16-ref {e:.4f}; in flight == single: {[_same(xs[k], singles[k]) for k in range(2)]}; "
          f"image 1 ~ image 0 {C.rel_rmse(singles[1], singles[0]):.3f}")
    assert e < 2e-2
    assert _same(xs[0], singles[0]) and _same(xs[1], singles[1])
    assert C.rel_rmse(singles[1], singles[0]) > 0.05


# ---- refusals on the engine -----------------------------------------------------------------------------------------------------------------
def test_engine_refusals_name_the_net(setup):
    s, m = setup, setup["tr"]
    lat = s["lat"].cuda()
    L = m._L
    out = torch.empty_like(lat)

    def refused(*words):
        rc = L.td_flux_forward(m._h, lat.data_ptr(), 0, out.data_ptr(), None)
        msg = L.td_last_error()
        assert rc == 2 and all(w.encode() in msg for w in words), (rc, msg)

    one = (ctypes.c_float * 1)(1.0)
    try:
        _attach(s, m, _two(s))
        # k beyond the attached count: both numbers
        assert L.td_flux_set_controlnet_scales_at(m._h, 2, ctypes.cast(one, ctypes.c_void_p), 1) == 2
        assert b"ControlNet 2 outside the 2 attached" in L.td_last_error()
        # net 1 prepared for another step count, then holding no control condition; at scale 0 it is not looked at
        b = s["cn"][1]["model"]
        _prepare(b, s["pe"], s["pool"], 3, control_mode=1)
        b.set_control_condition(s["cond2"].cuda())
        refused("ControlNet context 1 is prepared for 3 timesteps", "for 2")
        _prepare(b, s["pe"], s["pool"], 2, ids=R.latent_image_ids(4, 4), control_mode=1)
        _prepare(b, s["pe"], s["pool"], 2, control_mode=1)
        refused("attached ControlNet 1", "no control condition")
        m.set_controlnet_scales([0.0, 0.0], net=1)
        m.forward_step(lat, 0)
        m.set_controlnet_scales([1.0, 1.0], net=1)
        b.set_control_condition(s["cond2"].cuda())
        # reference tokens, whatever the attached count
        from kontext_common import reference_ids
        m.set_reference_tokens(torch.zeros(4, C.LAT, dtype=BF, device="cuda"), reference_ids(2, 2))
        refused("4 reference tokens")
        m.set_reference_tokens(None)
        m.forward_step(lat, 0)
    finally:
        m.attach_controlnets([])
        torch.cuda.synchronize()


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------------------
def test_pipeline_with_per_net_guidance_windows_equals_the_engine_run(setup):
    """128 x 128, 4 steps, scales [0.7, 0.45], control_guidance_start [0, 0.25], control_guidance_end [0.5, 1]: the tables
    [[.7, .7, 0, 0], [0, .45, .45, .45]]; latent-shaped control images are used as they are.  Against the engine given the same tables, in
    bits; and one union model listed twice (modes 0, 1) against the model and a loaded copy of it."""
    from thinkdiff.models import FluxControlNetPipelineRewritePrompt, FluxMultiControlNetModel
    from thinkdiff.models.flux_controlnet import controlnet_scale_tables
    from thinkdiff.models.flux_transformer import effective_scalar
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder
    s, m, N = setup, setup["tr"], 4
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(16, 16))
    dec.load_state_dict(V.init_weights(V.VaeConfig(), seed=12))
    a, b = s["cn"][0]["model"], s["cn"][1]["model"]
    g = torch.Generator().manual_seed(21)
    pe = torch.randn(1, 24, s["cfg"].joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(1, s["cfg"].pooled_projection_dim, generator=g).bfloat16().cuda()
    z = [torch.randn(1, 16, 16, 16, generator=_gen(4 + k), device="cuda", dtype=BF) for k in range(2)]
    lat0 = torch.randn(1, 64, C.LAT, generator=_gen(2), device="cuda", dtype=BF)
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pool, height=128, width=128, num_inference_steps=N, guidance_scale=3.5, output_type="latent",
              latents=lat0, control_image=z, controlnet_conditioning_scale=[SC0, SC1], control_guidance_start=[0.0, 0.25], control_guidance_end=[0.5, 1.0])
    tables = controlnet_scale_tables(N, 2, [SC0, SC1], [0.0, 0.25], [0.5, 1.0])
    assert tables == [[SC0, SC0, 0.0, 0.0], [0.0, SC1, SC1, SC1]] == M.scale_tables(N, 2, [SC0, SC1], [0.0, 0.25], [0.5, 1.0])
    pipe = FluxControlNetPipelineRewritePrompt(transformer=m, vae=dec, controlnet=FluxMultiControlNetModel([a, b]))
    got = pipe(control_mode=[None, 1], **kw).images
    assert m.attached_controlnets() == 0      # the transformer's contexts are left plain
    sig = R.make_sigmas(N, 64)
    t_eff = [effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]]
    ids = R.latent_image_ids(8, 8)
    try:
        m.set_condition(pe[0], pool[0], ids)
        m.set_timesteps(t_eff, G35)
        for cn, mode, zk in ((a, None, z[0]), (b, 1, z[1])):
            cn.set_condition(pe[0], pool[0], ids, control_mode=mode)
            cn.set_control_condition(_ops().flux_pack_latents(zk[0].contiguous()))
            cn.set_timesteps(t_eff, 0.0)
        m.attach_controlnets([a, b])
        for k in range(2):
            m.set_controlnet_scales(tables[k], net=k)
        x = lat0[0].clone()
        m.denoise(x, sig)
    finally:
        m.attach_controlnets([])
    torch.cuda.synchronize()
    assert _same(got[0], x)
    # scalar arguments apply to every net; both nets over the whole schedule move the result
    full = pipe(control_mode=[None, 1], **{**kw, "control_guidance_start": 0.0, "control_guidance_end": 1.0}).images
    assert not _same(full, got)
    # one model twice: the second appearance runs on its own fork
    u = s["cn"][1]
    copy = C.build_controlnet(u["cfg"], u["sd"], u["num_mode"])
    twice = FluxControlNetPipelineRewritePrompt(transformer=m, vae=dec, controlnet=FluxMultiControlNetModel([b, b]))(control_mode=[0, 1], **kw).images
    copies = FluxControlNetPipelineRewritePrompt(transformer=m, vae=dec, controlnet=FluxMultiControlNetModel([b, copy]))(control_mode=[0, 1], **kw).images
    assert _same(twice, copies) and not _same(twice, got)
