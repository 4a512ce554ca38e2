"""FLUX IP-Adapter on the GPU: td_ip_attention_bf16 against fp64, the per-context K / V arena, and the conditioned forward / loop / pipeline of the
tiny main model (oracle/flux_ref.tiny_config: D = 512, 2 double + 3 single blocks, 6 x 5 latent tokens, T = 11) against the test-local reference
tests/ip_adapter_common.py.

Bars.  Kernel: the project's attention bar (max error < 2^-7 of the output's scale, test_attention_gpu.py::_check) and rel-RMSE < 1.5 e_ref + 1e-3
with e_ref the distance of the bf16 torch restatement from the same fp64 reference, computed here (1.5: another accumulation order; 1e-3: the
bf16 output rounding).  Forward: the project's own (test_flux_controlnet_gpu.py): rel-RMSE < 2e-2 against the bf16 reference, < 1.5 e_ref + 2e-3
against the fp32 one; int8 as test_int8_mode_on_a_conditioned_engine; pixel RMSE < 1e-2.  What is an identity is held to bits."""
import ctypes

import pytest
import torch

import ip_adapter_common as C
from oracle import flux_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
S = C.H2 * C.W2
G35 = float((torch.tensor([3.5]).bfloat16() * 1000).float())


def _ops():
    from thinkdiff.ops import register
    return register()


def _i16(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_i16(a), _i16(b))


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def _kernel_case(rows, H, n_keys, k_mul, seed, with_norm):
    g = torch.Generator().manual_seed(seed)
    W = H * 128
    q = torch.randn(rows, W, generator=g).bfloat16()
    if not with_norm:
        q = (q * 0.7).bfloat16()
    k = (torch.randn(n_keys, W, generator=g) * k_mul).bfloat16()
    v = torch.randn(n_keys, W, generator=g).bfloat16()
    w = (1.0 + 0.1 * torch.randn(128, generator=g)).bfloat16() if with_norm else None
    return q, k, v, w


def _device_layout(q, k, v, H, extra_key_rows=0):
    """q at column 0 of a [rows + 3, 3 H 128] buffer, k / v in [n + extra, H 128 + 64] buffers, o in a [rows + 3, H 128 + 40] buffer preset to 7."""
    rows, n, W = q.shape[0], k.shape[0], H * 128
    Q = torch.randn(rows + 3, 3 * W, device="cuda").bfloat16()
    Q[:rows, :W] = q.cuda()
    K = torch.full((n + extra_key_rows, W + 64), 1e4, dtype=BF, device="cuda")
    V = torch.full((n + extra_key_rows, W + 64), 1e4, dtype=BF, device="cuda")
    K[:n, :W], V[:n, :W] = k.cuda(), v.cuda()
    O = torch.full((rows + 3, W + 40), 7.0, dtype=BF, device="cuda")
    return Q, K, V, O


KERNEL_CASES = [(1, 1, 1, 1.0), (77, 4, 4, 1.0), (77, 4, 20, 1.0), (257, 4, 128, 1.0), (257, 2, 129, 1.0), (77, 4, 256, 1.0),
                (77, 4, 16, 30.0), (257, 4, 128, 30.0)]


@pytest.mark.parametrize("with_norm,out_scale", [(True, 0.7), (False, 1.0)])
@pytest.mark.parametrize("rows,H,n_keys,k_mul", KERNEL_CASES)
def test_kernel_against_fp64(hip, rows, H, n_keys, k_mul, with_norm, out_scale):
    """Strided q (ldq = 3 H 128), wider k / v / o rows; x30 keys give scores of about +-130 and a near one-hot softmax: a score bound or a
    missing maximum overflows there.  Guard rows and columns stay; a second run repeats the bits."""
    q, k, v, w = _kernel_case(rows, H, n_keys, k_mul, rows * 7 + n_keys, with_norm)
    W = H * 128
    ref = C.kernel_reference(q, k, v, H, w, out_scale)
    e_ref = C.rel_rmse(C.kernel_restatement_bf16(q, k, v, H, w, out_scale), ref)
    Q, K, V, O = _device_layout(q, k, v, H)
    wd = w.cuda() if w is not None else None
    ip = _ops().ip_attention_
    ip(O[:rows, :W], Q[:rows, :W], K[:n_keys, :W], V[:n_keys, :W], H, wd, 1e-6, out_scale, False)
    got = O[:rows, :W].clone()
    ip(O[:rows, :W], Q[:rows, :W], K[:n_keys, :W], V[:n_keys, :W], H, wd, 1e-6, out_scale, False)
    fresh = _ops().ip_attention(Q[:rows, :W], K[:n_keys, :W], V[:n_keys, :W], H, wd, 1e-6, out_scale)
    torch.cuda.synchronize()
    assert _same(O[:rows, :W], got) and _same(fresh, got)
    assert bool((O[rows:] == 7.0).all()) and bool((O[:, W:] == 7.0).all())
    g = got.float().cpu()
    assert torch.isfinite(g).all()
    err_max = float((g.double() - ref).abs().max() / ref.abs().max())
    e = C.rel_rmse(g.double(), ref)
    print(f"({rows},{H},{n_keys}) k x{k_mul:g} norm={with_norm}: max err / scale {err_max:.3e}  rel-RMSE {e:.3e}  bf16 restatement {e_ref:.3e}")
    assert err_max < 2.0 ** -7
    assert e < 1.5 * e_ref + 1e-3


def test_kernel_padding_is_masked_and_accumulate_is_one_add(hip):
    """(77, 4, 20): key rows 20 .. 35, allocated and filled with 1e4, do not change a bit; accumulate == bf16(o + term) of the two single outputs."""
    rows, H, n = 77, 4, 20
    W = H * 128
    q, k, v, w = _kernel_case(rows, H, n, 1.0, 5, True)
    Q, K, V, _ = _device_layout(q, k, v, H, extra_key_rows=16)
    ip = _ops().ip_attention
    a = ip(Q[:rows, :W], K[:n, :W], V[:n, :W], H, w.cuda(), 1e-6, 0.7)
    tight = ip(Q[:rows, :W], k.cuda(), v.cuda(), H, w.cuda(), 1e-6, 0.7)
    q2, k2, v2, _ = _kernel_case(rows, H, 4, 1.0, 6, True)
    b = ip(Q[:rows, :W], k2.cuda(), v2.cuda(), H, w.cuda(), 1e-6, 0.4)
    acc = a.clone()
    _ops().ip_attention_(acc, Q[:rows, :W], k2.cuda(), v2.cuda(), H, w.cuda(), 1e-6, 0.4, True)
    torch.cuda.synchronize()
    assert bool((K[n:] == 1e4).all())
    assert _same(a, tight)
    assert _same(acc, (a.float() + b.float()).bfloat16())
    assert not _same(acc, a)


def test_kernel_refusals(hip):
    L = hip.lib()
    x = torch.zeros(64, 3 * 512 + 8, dtype=BF, device="cuda")
    kv = torch.zeros(300, 512, dtype=BF, device="cuda")
    o = torch.zeros(64, 512, dtype=BF, device="cuda")
    i64, f32 = ctypes.c_int64, ctypes.c_float

    def call(q_ptr, ldq, n_keys, H=4):
        return L.td_ip_attention_bf16(q_ptr, i64(ldq), kv.data_ptr(), kv.data_ptr(), i64(512), o.data_ptr(), i64(512), 64, H, n_keys, None, f32(1e-6), f32(1.0), 0, None)

    assert call(x.data_ptr(), 1536, 0) == 2 and b"n_keys=0" in L.td_last_error()
    assert call(x.data_ptr(), 1536, 257) == 2 and b"n_keys=257" in L.td_last_error()
    assert call(x.data_ptr() + 2, 1536, 4) == 2 and b"q must be 16-byte aligned" in L.td_last_error()
    assert call(x.data_ptr(), 1540, 4) == 2 and b"ldq=1540" in L.td_last_error()
    assert call(x.data_ptr(), 1536, 4, H=0) == 2
    assert call(x.data_ptr(), 1536, 4) == 0
    with pytest.raises(RuntimeError, match="H\\*128"):
        _ops().ip_attention(x[:, :256], kv[:4], kv[:4], 4, None, 1e-6, 1.0)
    torch.cuda.synchronize()


# ---- the tiny model -----------------------------------------------------------------------------------------------------------------------
def _prepare(m, pe, pool, n):
    from thinkdiff.models.flux_transformer import effective_scalar
    sig = R.make_sigmas(n, S)
    m.set_condition(pe.cuda(), pool.cuda(), R.latent_image_ids(C.H2, C.W2))
    m.set_timesteps([effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]], G35)
    return sig


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from kontext_common import build_engine
    cfg = C.main_config()
    sd = R.init_weights(cfg, seed=C.SEED_MAIN)
    lat, pe, pool = C.inputs(cfg, S, C.T_TXT)
    ip4, ip16 = C.ip_init_weights(cfg, 4, seed=C.SEED_IP), C.ip_init_weights(cfg, 16, seed=C.SEED_IP + 1)
    s = dict(cfg=cfg, sd=sd, tr=build_engine(cfg, sd), lat=lat, pe=pe, pool=pool, ip4=ip4, ip16=ip16,
             e1=C.image_embeds(1, 100), e1b=C.image_embeds(1, 101), e2=C.image_embeds(2, 102), refs={})
    return s


def _ref_forward(s, key, specs):
    """bf16 and fp32 reference of the one-step forward under `specs`, once per key."""
    if key not in s["refs"]:
        out = {}
        for tag, dtype in (("16", BF), ("32", torch.float32)):
            sd = {k: v.to(dtype) for k, v in s["sd"].items()}
            args = C.step_args(s["lat"], s["pe"], s["pool"], dtype, S, C.T_TXT)
            out[tag] = C.transformer_forward_ref(sd, s["cfg"], *args, adapters=C.make_adapters(s["cfg"], specs, dtype))
        s["refs"][key] = out
    return s["refs"][key]


@pytest.fixture()
def clean(setup):
    """Every engine test starts and ends without adapters."""
    m = setup["tr"]
    if m.ip_adapters():
        m.unload_ip_adapter()
    yield setup
    if m.ip_adapters():
        m.unload_ip_adapter()
    torch.cuda.synchronize()


# ---- 2. the K / V arena -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,emb", [("ip4", "e1"), ("ip16", "e2")])
def test_tokens_and_kv_match_the_restatement(clean, which, emb):
    """4 tokens x 1 image and 16 tokens x 2 images (32 keys): tokens and each block's K / V against the torch bf16 statements (GEMM tests' bar:
    max error < 2^-7 of the scale) and against the fp32 ones."""
    s, m = clean, clean["tr"]
    m.load_ip_adapter(s[which])
    m.set_ip_image_embeds(s[emb])
    w16, w32 = C.cast(s[which], BF), C.cast(s[which], torch.float32)
    t16, t32 = C.image_tokens(w16, s["cfg"], s[emb]), C.image_tokens(w32, s["cfg"], s[emb].float())
    got = m.read_ip(0).cpu()
    n_keys = s[emb].shape[0] * (4 if which == "ip4" else 16)
    assert got.shape == (n_keys, s["cfg"].joint_attention_dim)
    pairs = [("tokens", got, t16, t32)]
    for i in range(s["cfg"].num_layers):
        k16, v16 = C.block_kv(w16, i, t16)
        k32, v32 = C.block_kv(w32, i, t32)
        pairs += [(f"K{i}", m.read_ip(0, i, 0).cpu(), k16, k32), (f"V{i}", m.read_ip(0, i, 1).cpu(), v16, v32)]
    for name, g, r16, r32 in pairs:
        assert g.shape == r16.shape
        e16 = float((g.float() - r16.float()).abs().max() / r16.float().abs().max())
        e32, e_ref = C.rel_rmse(g, r32), C.rel_rmse(r16, r32)
        print(f"{which} {name}: max err / scale vs bf16 {e16:.3e}; rel-RMSE vs fp32 {e32:.3e} (bf16 statements {e_ref:.3e})")
        assert e16 < 2.0 ** -7
        assert e32 < 1.5 * e_ref + 2e-3


# ---- 3. one forward step ------------------------------------------------------------------------------------------------------------------
def _check_forward(v, ref, what):
    e16, e32, e_ref = C.rel_rmse(v[None], ref["16"]), C.rel_rmse(v[None], ref["32"]), C.rel_rmse(ref["16"], ref["32"])
    print(f"{what}: hip~bf16-ref {e16:.4f}  hip~fp32-ref {e32:.4f}  bf16~fp32 ref {e_ref:.4f}")
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3


def test_forward_single_adapter(clean):
    s, m = clean, clean["tr"]
    _prepare(m, s["pe"], s["pool"], 2)
    lat = s["lat"].cuda()
    v_plain = m.forward_step(lat, 0).clone()
    m.load_ip_adapter(s["ip4"])
    m.set_ip_adapter_scale(C.SCALE)
    m.set_ip_image_embeds(s["e1"])
    v = m.forward_step(lat, 0).clone()
    m.set_ip_image_embeds(s["e1b"])
    v_other = m.forward_step(lat, 0).clone()
    torch.cuda.synchronize()
    _check_forward(v, _ref_forward(s, "single", [(s["ip4"], s["e1"], C.SCALE)]), "one adapter, 4 tokens, scale 0.7")
    d_plain, d_other = C.rel_rmse(v_plain, v), C.rel_rmse(v_other, v)
    print(f"moved by: no image prompt {d_plain:.3f}  another image {d_other:.3f}")
    assert d_plain > 0.1 and d_other > 0.1


def test_forward_two_adapters_and_per_block_scale(clean):
    s, m = clean, clean["tr"]
    _prepare(m, s["pe"], s["pool"], 2)
    lat = s["lat"].cuda()
    m.load_ip_adapter(s["ip4"])
    m.load_ip_adapter(s["ip16"])
    m.set_ip_adapter_scale([C.SCALE, 0.4])
    m.set_ip_image_embeds([s["e1"], s["e2"]])
    v2 = m.forward_step(lat, 0).clone()
    m.set_ip_adapter_scale([[0.0, C.SCALE], 0.0])
    v_blk = m.forward_step(lat, 0).clone()
    torch.cuda.synchronize()
    _check_forward(v2, _ref_forward(s, "two", [(s["ip4"], s["e1"], C.SCALE), (s["ip16"], s["e2"], 0.4)]), "two adapters (4 and 2 x 16 tokens), 0.7 / 0.4")
    _check_forward(v_blk, _ref_forward(s, "blk", [(s["ip4"], s["e1"], [0.0, C.SCALE])]), "per-block scale [0, 0.7]")
    assert C.rel_rmse(v_blk, v2) > 0.05


# ---- 4. identities ------------------------------------------------------------------------------------------------------------------------
def _traced(m, lat):
    m.trace_begin(400)
    v = m.forward_step(lat, 0).clone()
    tr = m.trace_end()
    return v, sum(c["launches"] for c in tr.values())


def test_parent_identities_and_launch_counts(clean):
    s, m = clean, clean["tr"]
    _prepare(m, s["pe"], s["pool"], 2)
    lat = s["lat"].cuda()
    v0, n0 = _traced(m, lat)
    m.load_ip_adapter(s["ip4"])
    v_loaded, n_loaded = _traced(m, lat)                     # loaded, no embeds
    m.set_ip_image_embeds(s["e1"])
    v_on, n_on = _traced(m, lat)
    m.set_ip_adapter_scale(0.0)
    v_zero, n_zero = _traced(m, lat)                         # all scales 0
    m.set_ip_adapter_scale(1.0)
    m.set_ip_image_embeds(None)
    v_cleared, n_cleared = _traced(m, lat)                   # set, then cleared
    m.set_ip_image_embeds(s["e1"])
    m.unload_ip_adapter()
    v_unloaded, n_unloaded = _traced(m, lat)
    torch.cuda.synchronize()
    assert not _same(v_on, v0)
    for v, n in ((v_loaded, n_loaded), (v_zero, n_zero), (v_cleared, n_cleared), (v_unloaded, n_unloaded)):
        assert _same(v, v0) and n == n0
    L = s["cfg"].num_layers
    print(f"launches: plain {n0}, one active slot {n_on} (+{n_on - n0} over {L} double blocks)")
    assert n0 < n_on <= n0 + 2 * L


# ---- 5. contexts --------------------------------------------------------------------------------------------------------------------------
def test_contexts_in_flight_and_replaced_embeds(clean):
    s, m = clean, clean["tr"]
    n = 3
    m.load_ip_adapter(s["ip4"])
    m.set_ip_adapter_scale(C.SCALE)
    singles = []
    for e in (s["e1"], s["e1b"]):
        sig = _prepare(m, s["pe"], s["pool"], n)
        m.set_ip_image_embeds(e)
        x = s["lat"].cuda().clone()
        m.denoise(x, sig)
        singles.append(x)
    fork = m.fork()
    ctxs, streams = [m, fork], [torch.cuda.Stream(), torch.cuda.Stream()]
    xs = [s["lat"].cuda().clone() for _ in range(2)]
    torch.cuda.synchronize()
    try:
        for ctx, e in zip(ctxs, (s["e1"], s["e1b"])):
            sig = _prepare(ctx, s["pe"], s["pool"], n)
            ctx.set_ip_image_embeds(e)
        torch.cuda.synchronize()
        type(m).denoise_multi(ctxs, xs, sig, streams)
        torch.cuda.synchronize()
        assert _same(xs[0], singles[0]) and _same(xs[1], singles[1])
        assert C.rel_rmse(singles[1], singles[0]) > 0.05
        # new embeds on a context replace the old K / V: the fork, holding e1b, takes e1 and equals the context that always held it
        fork.set_ip_image_embeds(s["e1"])
        y = s["lat"].cuda().clone()
        fork.denoise(y, sig)
        torch.cuda.synchronize()
        assert _same(y, singles[0])
    finally:
        fork.set_ip_image_embeds(None)
    # the 3-step loop against the reference loop
    ref = C.denoise_ref(s["sd"], s["cfg"], s["lat"][None], s["pe"][None], s["pool"][None], C.H2, C.W2, n,
                        C.make_adapters(s["cfg"], [(s["ip4"], s["e1"], C.SCALE)]))
    e = C.rel_rmse(singles[0][None], ref)
    print(f"3-step denoise with an image prompt: hip~bf16-ref {e:.4f}")
    assert e < 2e-2


# ---- 6. the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_pipeline_with_image_embeds(clean):
    """128 x 128 (8 x 8 latent tokens), 2 steps, num_images_per_prompt = 2 (both images in flight, the same image prompt), tiny VAE."""
    from oracle import vae_ref as V
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder
    s, m = clean, clean["tr"]
    n = 2
    vcfg = V.VaeConfig()
    sd_dec = V.init_weights(vcfg, seed=12)
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(16, 16))
    dec.load_state_dict(sd_dec)
    pipe = FluxPipelineRewritePrompt(transformer=m, vae=dec)
    pipe.load_ip_adapter(s["ip4"])
    pipe.set_ip_adapter_scale(C.SCALE)
    gen = lambda: torch.Generator(device="cuda").manual_seed(8)
    kw = dict(prompt_embeds=s["pe"][None].cuda(), pooled_prompt_embeds=s["pool"][None].cuda(), height=128, width=128,
              num_inference_steps=n, guidance_scale=3.5, num_images_per_prompt=2)
    emb = s["e1"][None].cuda()
    out = pipe(ip_adapter_image_embeds=emb, generator=gen(), output_type="latent", **kw).images
    px = pipe(ip_adapter_image_embeds=emb, generator=gen(), output_type="np", **kw).images
    plain = pipe(generator=gen(), output_type="latent", **kw).images
    torch.cuda.synchronize()
    noise = torch.randn((2, 16, 16, 16), generator=gen(), device="cuda", dtype=BF).cpu()
    ad = C.make_adapters(s["cfg"], [(s["ip4"], s["e1"], C.SCALE)])
    for b in range(2):
        x = C.denoise_ref(s["sd"], s["cfg"], R.pack_latents(noise[b:b + 1]), s["pe"][None], s["pool"][None], 8, 8, n, ad)
        _, ref_u8 = V.latents_to_image(sd_dec, vcfg, x, 16, 16)
        rel = C.rel_rmse(out[b], x[0])
        prmse = float(((px[b].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
        d = C.rel_rmse(plain[b], out[b])
        print(f"pipeline image {b}: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}; moved by the image prompt {d:.3f}")
        assert rel < 2e-2 and prmse < 1e-2
        assert d > 0.05
    # the call after one with an image prompt is the plain model again (the contexts' prompts are cleared), also once the adapter is gone: to bits
    pipe.unload_ip_adapter()
    again = pipe(generator=gen(), output_type="latent", **kw).images
    torch.cuda.synchronize()
    assert _same(again, plain)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe(ip_adapter_image_embeds=emb, generator=gen(), output_type="latent", **kw)
    with pytest.raises(NotImplementedError, match="negative"):
        pipe(negative_ip_adapter_image_embeds=emb, generator=gen(), output_type="latent", **kw)


# ---- 7. 8-bit modes -----------------------------------------------------------------------------------------------------------------------
def test_int8_smoothing_and_fp8_attention(clean):
    """int8 Linears with smoothing + the e4m3 attention, one step (behind the calibration forward), against the reference configured the same way
    (int8 block Linears -- to_q among them --, 8-bit attention; the adapter's Linears and the IP attention stay bf16, as on the engine) under
    test_int8_mode_on_a_conditioned_engine's bars.  The same mode's plain distances are printed beside them: the IP term is bf16, it does not
    widen the distance."""
    s, m = clean, clean["tr"]
    _prepare(m, s["pe"], s["pool"], 2)
    lat = s["lat"].cuda()
    m.load_ip_adapter(s["ip4"])
    m.set_ip_adapter_scale(C.SCALE)
    args = C.step_args(s["lat"], s["pe"], s["pool"], BF, S, C.T_TXT)
    ad = C.make_adapters(s["cfg"], [(s["ip4"], s["e1"], C.SCALE)])
    ref16, ref16_plain = _ref_forward(s, "single", [(s["ip4"], s["e1"], C.SCALE)])["16"], R.transformer_forward(s["sd"], s["cfg"], *args)
    R.INT8_BLOCK_LINEARS = R.FP8_ATTENTION = True
    try:
        ref8 = C.transformer_forward_ref(s["sd"], s["cfg"], *args, adapters=ad)
        ref8_plain = R.transformer_forward(s["sd"], s["cfg"], *args)
    finally:
        R.INT8_BLOCK_LINEARS = R.FP8_ATTENTION = False

    def both():
        m.set_ip_image_embeds(None)
        a = m.forward_step(lat, 0).clone()
        m.set_ip_image_embeds(s["e1"])
        return a, m.forward_step(lat, 0).clone()

    p16, i16 = both()
    try:
        m.set_precision("int8", smoothing=True)
        m.set_attention("fp8")
        m.forward_step(lat, 0)                      # the calibration forward (with the image prompt set)
        p8, i8 = both()
    finally:
        m.set_attention("bf16")
        m.set_precision("bf16")
    back = m.forward_step(lat, 0).clone()
    torch.cuda.synchronize()
    e16, e88, d_hip, d_ref = C.rel_rmse(i16[None], ref16), C.rel_rmse(i8[None], ref8), C.rel_rmse(i8, i16), C.rel_rmse(ref8, ref16)
    pe88, pd_hip, pd_ref = C.rel_rmse(p8[None], ref8_plain), C.rel_rmse(p8, p16), C.rel_rmse(ref8_plain, ref16_plain)
    print(f"with image prompt: hip~bf16-ref {e16:.4f}  hip-8bit~ref-8bit {e88:.4f}  8bit~bf16 hip {d_hip:.4f} ref {d_ref:.4f}")
    print(f"plain, same mode:                          hip-8bit~ref-8bit {pe88:.4f}  8bit~bf16 hip {pd_hip:.4f} ref {pd_ref:.4f}")
    assert torch.isfinite(i8.float()).all()
    assert e16 < 2e-2 and e88 < 2e-2
    assert d_hip < 3e-2 and abs(d_hip - d_ref) < 0.5 * d_ref + 2e-3
    assert C.rel_rmse(i8, p8) > 0.1
    assert _same(back, i16)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(m, lat, *words):
    L = m._L
    out = torch.empty_like(lat)
    rc = L.td_flux_forward(m._h, lat.data_ptr(), 0, out.data_ptr(), None)
    msg = L.td_last_error()
    assert rc == 2 and all(w.encode() in msg for w in words), (rc, msg)


def test_engine_refusals(clean):
    import controlnet_common as CN
    from kontext_common import reference_ids
    s, m = clean, clean["tr"]
    L = m._L
    lat = s["lat"].cuda()
    _prepare(m, s["pe"], s["pool"], 2)
    m.load_ip_adapter(s["ip4"])
    m.set_ip_image_embeds(s["e1"])
    # reference tokens
    m.set_reference_tokens(s["lat"][:6].cuda(), reference_ids(2, 3))
    _refused(m, lat, "reference tokens", "slot 0")
    m.set_reference_tokens(None)
    # an attached ControlNet
    cfg_cn = CN.cn_config(1, 0)
    cn = CN.build_controlnet(cfg_cn, CN.cn_init_weights(cfg_cn, 0, seed=7))
    m.attach_controlnet(cn)
    try:
        _refused(m, lat, "ControlNet is attached")
    finally:
        m.attach_controlnet(None)
    # a stale epoch: a parameter of the slot is loaded again
    w = s["ip4"]["image_proj"]["norm.bias"].cuda()
    _ops().flux_ip_adapter_load_param(int(m._h.value), 0, "image_proj.norm.bias", w)
    _refused(m, lat, "weights of IP-Adapter slot 0 changed")
    m.set_ip_image_embeds(s["e1"])
    assert L.td_flux_forward(m._h, lat.data_ptr(), 0, torch.empty_like(lat).data_ptr(), None) == 0
    # too many keys: 65 images x 4 tokens
    with pytest.raises(RuntimeError, match="65 images x 4 tokens = 260 keys"):
        m.set_ip_image_embeds(C.image_embeds(65, 1))
    # model-level calls on a fork, and on a ControlNet
    fork = m.fork()
    slot = ctypes.c_int()
    assert L.td_flux_ip_adapter_add(fork._h, 4, 32, ctypes.byref(slot)) == 2 and b"parent context" in L.td_last_error()
    assert L.td_flux_ip_adapter_remove(fork._h, 0) == 2 and b"parent context" in L.td_last_error()
    one = (ctypes.c_float * 1)(0.5)
    assert L.td_flux_set_ip_adapter_scale(fork._h, 0, ctypes.cast(one, ctypes.c_void_p), 1) == 2
    assert L.td_flux_ip_adapter_add(cn._h, 4, 32, ctypes.byref(slot)) == 2 and b"ControlNet" in L.td_last_error()
    # unknown names, wrong counts, free slots
    assert L.td_flux_ip_adapter_load_param(m._h, 0, b"ip_adapter.2.to_k_ip.weight", w.data_ptr(), ctypes.c_int64(8), None) == 2 and b"unknown parameter" in L.td_last_error()
    assert L.td_flux_ip_adapter_load_param(m._h, 0, b"image_proj.norm.bias", w.data_ptr(), ctypes.c_int64(8), None) == 2 and b"expects 512 elements" in L.td_last_error()
    assert L.td_flux_set_ip_image_embeds(m._h, 1, w.data_ptr(), 1, None) == 2 and b"slot 1 holds no adapter" in L.td_last_error()
    three = (ctypes.c_float * 3)(1, 1, 1)
    assert L.td_flux_set_ip_adapter_scale(m._h, 0, ctypes.cast(three, ctypes.c_void_p), 3) == 2 and b"3 scales" in L.td_last_error()
    torch.cuda.synchronize()
