"""FLUX.1 Kontext on the GPU: tiny transformers (oracle/flux_ref.tiny_config, 1 + 1 blocks) and the full FLUX.1 VAE architecture with
seeded weights, as test_flux_fill_gpu.py builds them.

The reference tokens move the first S output rows of these tiny models by less than the 2e-2 parity bar (0.3 - 1.0 % rel-RMSE, measured on
the oracle alone), so parity with the oracle cannot show that they are wired.  What discriminates is BITS against the path the engine
already had: the plain forward over `cat([latents, ref])` with `cat([ids, ref_ids])`, sliced (composition "B" below).  Bars that are
tolerances are the project's own: forward / denoise vs the bf16 oracle rel-RMSE < 2e-2, vs the fp32 oracle < 1.5 e_ref + 2e-3, fp8 vs
the fp8 oracle < 3e-2, int8 vs the int8 oracle < 2e-2, VAE moments / image rel-RMSE < 3e-2, pixel RMSE < 1e-2."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kontext_common import LAT, build_engine, denoise_ref, forward_ref, reference_ids
from oracle import flux_ref as R
from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, nhwc_moments_to_nchw, preprocess_u8

pytestmark = pytest.mark.gpu

SCALING, SHIFT = 0.3611, 0.1159
BF = torch.bfloat16


def _ops():
    from thinkdiff.ops import register
    return register()


def _i16(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_i16(a), _i16(b))


def _rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _image(H, W, seed):
    from PIL import Image
    u8 = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    u8 = F.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return Image.fromarray(u8.numpy()), u8


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from thinkdiff.models import FluxKontextPipelineRewritePrompt, FluxPipelineRewritePrompt
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder, AutoencoderKLEncoder
    cfg = R.tiny_config(num_layers=1, num_single_layers=1)
    sd = R.init_weights(cfg, seed=4)
    tr = build_engine(cfg, sd)
    vcfg = V.VaeConfig()
    sd_dec, sd_enc = V.init_weights(vcfg, seed=12), encoder_init_weights(vcfg, seed=13)
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(32, 32))
    dec.load_state_dict(sd_dec)
    enc = AutoencoderKLEncoder(AutoencoderKLConfig(), max_image_size=(256, 256))
    enc.load_state_dict(sd_enc)
    g = torch.Generator().manual_seed(21)
    return dict(cfg=cfg, sd=sd, tr=tr, vcfg=vcfg, sd_dec=sd_dec, sd_enc=sd_enc, enc=enc, dec=dec,
                pipe=FluxKontextPipelineRewritePrompt(transformer=tr, vae=dec, vae_encoder=enc),
                t2i=FluxPipelineRewritePrompt(transformer=tr, vae=dec),
                pe=torch.randn(2, 24, cfg.joint_attention_dim, generator=g).bfloat16().cuda(),
                pool=torch.randn(2, cfg.pooled_projection_dim, generator=g).bfloat16().cuda(),
                npe=torch.randn(1, 17, cfg.joint_attention_dim, generator=g).bfloat16().cuda(),
                npool=torch.randn(1, cfg.pooled_projection_dim, generator=g).bfloat16().cuda())


def _inputs(cfg, S, S_ref, T, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(S, LAT, generator=g).bfloat16()
    ref = torch.randn(S_ref, LAT, generator=g).bfloat16()
    pe = torch.randn(T, cfg.joint_attention_dim, generator=g).bfloat16()
    pool = torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16()
    return lat, ref, pe, pool


def _prepare(m, pe, pool, ids, n, S_sched):
    """set_condition + the schedule of `S_sched` latent tokens (the latents' own count, also for composition B)."""
    from thinkdiff.models.flux_transformer import effective_scalar
    sig = R.make_sigmas(n, S_sched)
    m.set_condition(pe.cuda(), pool.cuda(), ids)
    m.set_timesteps([effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]], float((torch.tensor([3.5]).bfloat16() * 1000).float()))
    return sig


# ---- 1. reference tokens == the long-sequence forward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("h2,w2,rh2,rw2,T", [(8, 8, 8, 8, 24), (12, 20, 8, 12, 65), (8, 8, 12, 20, 24)])
def test_reference_tokens_equal_the_long_sequence_forward(setup, h2, w2, rh2, rw2, T):
    """A = set_condition(ids), set_reference_tokens(ref, ref_ids), forward_step(lat).  B = the composition the engine could always run:
    set_condition(cat(ids, ref_ids)), forward_step(cat(lat, ref))[:S].  A equals B bit for bit, or is no further from B than B is from the
    bf16 oracle (proj_out runs over fewer rows in A: the launcher may pick another tile); which held is printed.  On the MI355X the first
    two cases held bit for bit; at (64, 240, 24) a few values differ in the last bit (A~B < 5e-7 against B~oracle 1.8e-3): DESIGN.md 5.4."""
    s = setup
    cfg, sd, m = s["cfg"], s["sd"], s["tr"]
    S, Sr = h2 * w2, rh2 * rw2
    lat, ref, pe, pool = _inputs(cfg, S, Sr, T, seed=S + Sr + T)
    ids, rid = R.latent_image_ids(h2, w2), reference_ids(rh2, rw2)
    latc, refc = lat.cuda(), ref.cuda()
    # B, and the plain forward
    _prepare(m, pe, pool, torch.cat([ids, rid]), 2, S)
    vB = m.forward_step(torch.cat([latc, refc]).contiguous(), 0)[:S].clone()
    _prepare(m, pe, pool, ids, 2, S)
    plain = m.forward_step(latc, 0).clone()
    # A
    m.set_reference_tokens(refc, rid)
    vA = m.forward_step(latc, 0).clone()
    n_ref = ctypes.c_int(-1)
    assert m._L.td_flux_reference_tokens(m._h, ctypes.byref(n_ref)) == 0 and n_ref.value == Sr
    # inequalities of bits: permuted reference rows, first id coordinate 0, no reference
    m.set_reference_tokens(refc.flip(0).contiguous(), rid)
    v_perm = m.forward_step(latc, 0).clone()
    rid0 = rid.clone()
    rid0[:, 0] = 0
    m.set_reference_tokens(refc, rid0)
    v_id0 = m.forward_step(latc, 0).clone()
    m.set_reference_tokens(None)
    v_clear = m.forward_step(latc, 0).clone()
    m.set_reference_tokens(refc, rid)
    again = m.forward_step(latc, 0).clone()
    _prepare(m, pe, pool, ids, 2, S)                      # a fresh set_condition voids the reference tokens
    v_fresh = m.forward_step(latc, 0).clone()
    assert m._L.td_flux_reference_tokens(m._h, ctypes.byref(n_ref)) == 0 and n_ref.value == 0
    torch.cuda.synchronize()
    # oracles of B
    t, g = torch.tensor([float(R.make_sigmas(2, S)[0]) * 1000.0]).bfloat16() / 1000, torch.tensor([3.5])      # the pipeline's t / 1000, in bf16
    args = lambda f: (pe[None].to(f), pool[None].to(f))
    ref16 = forward_ref(sd, cfg, lat[None], ref[None], *args(BF), t.bfloat16(), ids.bfloat16(), rid.bfloat16(), torch.zeros(T, 3).bfloat16(), g)
    sd32 = {k: v.float() for k, v in sd.items()}
    ref32 = forward_ref(sd32, cfg, lat[None].float(), ref[None].float(), *args(torch.float32), t.bfloat16().float(), ids, rid, torch.zeros(T, 3),
                        torch.tensor([float((g.bfloat16() * 1000).float()) / 1000]))
    exact = _same(vA, vB)
    d_ab, e16, e32, e_ref = _rel_rmse(vA, vB), _rel_rmse(vB[None], ref16), _rel_rmse(vB[None], ref32), _rel_rmse(ref16, ref32)
    print(f"S {S} S_ref {Sr} T {T}: A == B bit for bit: {exact};  A~B {d_ab:.6f}  B~bf16-oracle {e16:.4f}  B~fp32-oracle {e32:.4f}  "
          f"bf16~fp32 oracle {e_ref:.4f};  moved by: permuted {_rel_rmse(v_perm, vA):.4f}  id0 {_rel_rmse(v_id0, vA):.4f}  none {_rel_rmse(plain, vA):.4f}")
    assert vA.shape == (S, LAT)
    assert exact or d_ab <= e16
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3
    assert _same(again, vA)
    assert not _same(v_perm, vA) and not _same(v_id0, vA) and not _same(plain, vA)
    assert _same(v_clear, plain) and _same(v_fresh, plain)


def test_reference_token_refusals(setup):
    s = setup
    cfg, m = s["cfg"], s["tr"].fork()
    lat, ref, pe, pool = _inputs(cfg, 64, 64, 24, seed=2)
    rid = reference_ids(8, 8)
    with pytest.raises(RuntimeError, match="no condition"):
        m.set_reference_tokens(ref.cuda(), rid)
    _prepare(m, pe, pool, R.latent_image_ids(8, 8), 2, 64)
    with pytest.raises(RuntimeError, match=r"\[64, 3\]"):
        m.set_reference_tokens(ref.cuda(), rid[:32])
    with pytest.raises(RuntimeError, match="S_img=64 \\+ S_ref=480 exceed the image-stream capacity 512"):
        m.set_reference_tokens(torch.zeros(480, LAT, dtype=BF, device="cuda"), torch.zeros(480, 3))
    m.set_reference_tokens(torch.zeros(448, LAT, dtype=BF, device="cuda"), torch.zeros(448, 3))      # exactly the capacity
    out = m.forward_step(lat.cuda(), 0)
    torch.cuda.synchronize()
    assert out.shape == (64, LAT) and torch.isfinite(out.float()).all()
    # a channel-conditioned engine takes none
    from fill_common import build_engine as build_cond, conditioned_weights
    ccfg, _, eng = conditioned_weights(128, 5)
    c = build_cond(ccfg, eng)
    c.set_condition(torch.zeros(24, ccfg.joint_attention_dim, dtype=BF, device="cuda"), torch.zeros(ccfg.pooled_projection_dim, dtype=BF, device="cuda"),
                    R.latent_image_ids(8, 8))
    with pytest.raises(RuntimeError, match="channel-conditioned"):
        c.set_reference_tokens(ref.cuda(), rid)


# ---- 2. the denoise loop -------------------------------------------------------------------------------------------------------------
def _compose_B(m, lat, ref, pe, pool, ids, rid, n, sig):
    """The hand composition over B's forwards: per step cat, the plain forward over S + S_ref rows, slice, euler_step_ on the first S rows."""
    S = lat.shape[0]
    _prepare(m, pe, pool, torch.cat([ids, rid]), n, S)
    x = lat.clone()
    for i in range(n):
        v = m.forward_step(torch.cat([x, ref]).contiguous(), i)[:S].contiguous()
        _ops().euler_step_(x, v, float(sig[i + 1] - sig[i]))
    return x


@pytest.mark.parametrize("h2,w2,rh2,rw2,T", [(8, 8, 8, 8, 24), (12, 20, 8, 12, 65)])
def test_denoise_with_reference_tokens(setup, h2, w2, rh2, rw2, T):
    s = setup
    cfg, sd, m = s["cfg"], s["sd"], s["tr"]
    S, Sr, n = h2 * w2, rh2 * rw2, 4
    lat, ref, pe, pool = _inputs(cfg, S, Sr, T, seed=3 * S + Sr)
    ids, rid = R.latent_image_ids(h2, w2), reference_ids(rh2, rw2)
    sig = R.make_sigmas(n, S)
    xB = _compose_B(m, lat.cuda(), ref.cuda(), pe, pool, ids, rid, n, sig)
    _prepare(m, pe, pool, ids, n, S)
    m.set_reference_tokens(ref.cuda(), rid)
    xA = lat.cuda().clone()
    m.denoise(xA, sig)
    torch.cuda.synchronize()
    want = denoise_ref(sd, cfg, lat[None], ref[None], rid, pe[None], pool[None], h2, w2, n)
    exact = _same(xA, xB)
    d_ab, d_b, d_a = _rel_rmse(xA, xB), _rel_rmse(xB[None], want), _rel_rmse(xA[None], want)
    print(f"4-step denoise S {S} S_ref {Sr}: A == B bit for bit: {exact};  A~B {d_ab:.6f}  B~oracle {d_b:.4f}  A~oracle {d_a:.4f}")
    assert exact or d_ab <= d_b
    assert d_a < 2e-2


# ---- 3. images in flight (through the pipeline) ------------------------------------------------------------------------------------------
def _kw(s, **over):
    kw = dict(prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=128, width=128, max_area=128 ** 2, num_inference_steps=4,
              guidance_scale=3.5, _auto_resize=False)
    kw.update(over)
    return kw


def test_images_in_flight_and_reference_per_context(setup):
    s = setup
    p = s["pipe"]
    imgA, imgB = _image(128, 192, 11)[0], _image(96, 160, 12)[0]
    kw = _kw(s, output_type="latent")
    old = p.images_in_flight
    try:
        runs = {}
        for G in (1, 2):
            p.images_in_flight = G
            runs[G] = p(image=imgA, num_images_per_prompt=3, generator=_gen(5), **kw).images.clone()
        lat = torch.randn(2, 64, LAT, generator=torch.Generator().manual_seed(6)).to(BF).cuda()
        p.images_in_flight = 2
        both = p(image=[imgA, imgB], num_images_per_prompt=2, latents=lat, **kw).images.clone()
        singles = [p(image=im, latents=lat[b:b + 1], **kw).images[0].clone() for b, im in enumerate((imgA, imgB))]
        other = p(image=imgA, latents=lat[1:2], **kw).images[0].clone()
    finally:
        p.images_in_flight = old
    torch.cuda.synchronize()
    assert runs[1].shape == (3, 64, LAT) and _same(runs[1], runs[2])
    assert not _same(runs[1][0], runs[1][1])
    assert _same(both[0], singles[0]) and _same(both[1], singles[1])
    assert not _same(both[1], other)      # sample 1 read the second image's tokens, not the first's


# ---- 4. the 8-bit modes on a context with reference tokens ---------------------------------------------------------------------------------
def _eightbit_case(setup):
    s = setup
    cfg, m = s["cfg"], s["tr"]
    h2, w2, rh2, rw2, T = 12, 20, 8, 12, 65
    S, Sr = h2 * w2, rh2 * rw2
    lat, ref, pe, pool = _inputs(cfg, S, Sr, T, seed=77)
    ids, rid = R.latent_image_ids(h2, w2), reference_ids(rh2, rw2)
    t, g = torch.tensor([float(R.make_sigmas(2, S)[0]) * 1000.0]).bfloat16() / 1000, torch.tensor([3.5])      # the pipeline's t / 1000, in bf16
    ref_args = (s["sd"], cfg, lat[None], ref[None], pe[None], pool[None], t.bfloat16(), ids.bfloat16(), rid.bfloat16(), torch.zeros(T, 3).bfloat16(), g)

    def run():
        _prepare(m, pe, pool, ids, 2, S)
        m.set_reference_tokens(ref.cuda(), rid)
        return m.forward_step(lat.cuda(), 0)[None].clone()
    return m, ref_args, run


def test_fp8_mode_with_reference_tokens(setup):
    m, ref_args, run = _eightbit_case(setup)
    R.FP8_BLOCK_LINEARS = True
    try:
        ref8 = forward_ref(*ref_args)
    finally:
        R.FP8_BLOCK_LINEARS = False
    out16 = run()
    try:
        m.set_precision("fp8")
        out8 = run()
    finally:
        m.set_precision("bf16")
    back = run()
    torch.cuda.synchronize()
    e88 = _rel_rmse(out8, ref8)
    print(f"reference tokens, fp8: hip-fp8~oracle-fp8 {e88:.4f}   hip-fp8~hip-bf16 {_rel_rmse(out8, out16):.4f}")
    assert e88 < 3e-2
    assert _same(back, out16)


def test_int8_mode_with_reference_tokens(setup):
    m, ref_args, run = _eightbit_case(setup)
    R.INT8_BLOCK_LINEARS = True
    try:
        ref8 = forward_ref(*ref_args)
    finally:
        R.INT8_BLOCK_LINEARS = False
    try:
        m.set_precision("int8")
        out8 = run()
    finally:
        m.set_precision("bf16")
    torch.cuda.synchronize()
    e88 = _rel_rmse(out8, ref8)
    print(f"reference tokens, int8: hip-int8~oracle-int8 {e88:.4f}")
    assert e88 < 2e-2


def test_int8_smoothing_history_fp8_attention_with_reference_tokens(setup):
    """int8 + smoothing + fp8 attention with dynamic and with history scales over a 4-step denoise on a context with reference tokens:
    finite, repeatable bit for bit, history tracking dynamic by test_int8_history_scales_track_the_dynamic_path's inequality, and a second
    image's reference tokens do not meet the first image's per-token history."""
    s = setup
    cfg, m = s["cfg"], s["tr"]
    h2 = w2 = 16
    S, Sr, T, n = 256, 96, 40, 4
    lat, _, pe, pool = _inputs(cfg, S, Sr, T, seed=3)
    g = torch.Generator().manual_seed(8)
    refs = [torch.randn(Sr, LAT, generator=g).bfloat16().cuda() for _ in range(2)]
    ids, rid = R.latent_image_ids(h2, w2), reference_ids(8, 12)
    sig = _prepare(m, pe, pool, ids, n, S)

    def run(ref):
        m.set_reference_tokens(ref, rid)
        x = lat.cuda().clone()
        m.denoise(x, sig)
        torch.cuda.synchronize()
        return x.float().cpu()

    outs = {}
    try:
        outs["bf16"] = run(refs[0])
        m.set_attention("fp8")
        for name, kw in (("dynamic", dict(precision="int8", smoothing=True)), ("history", dict(precision="int8", smoothing=True, act_scales="history")),
                         ("history2", dict(precision="int8", smoothing=True, act_scales="history"))):
            m.set_precision(**kw)
            outs[name] = run(refs[0])
        second_after_first = run(refs[1])
        m.set_precision("int8", smoothing=True, act_scales="history")      # forgets the calibration and the history: a fresh start
        run(refs[1])                                                       # (the calibration forward is part of a first run)
        outs["first"] = run(refs[0])
        second_after_first2 = run(refs[1])
        # the discriminator for the setter's history reset: step 1 reads the per-token history step 0 left.  a: image B's own history;
        # b: step 1 of image B with no predecessor (the mode-0 path); c: step 0 ran on image A, then B's tokens were set.  c must be b.
        x0 = lat.cuda()

        def step1(first, with_step0):
            _prepare(m, pe, pool, ids, n, S)
            m.set_reference_tokens(first, rid)
            if with_step0:
                m.forward_step(x0, 0)
            if first is not refs[1]:
                m.set_reference_tokens(refs[1], rid)
            return m.forward_step(x0, 1).clone()
        h_a, h_b, h_c = step1(refs[1], True), step1(refs[1], False), step1(refs[0], True)
        torch.cuda.synchronize()
    finally:
        m.set_attention("bf16")
        m.set_precision("bf16")
    rel = lambda a, b: float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    d_int8, d_hist, d_hd = rel(outs["dynamic"], outs["bf16"]), rel(outs["history"], outs["bf16"]), rel(outs["history"], outs["dynamic"])
    print(f"reference tokens, 4-step denoise, int8 + smoothing + fp8 attention: dynamic~bf16 {d_int8:.4f}  history~bf16 {d_hist:.4f}  history~dynamic {d_hd:.4f}")
    assert all(torch.isfinite(v).all() for v in outs.values())
    assert torch.equal(outs["history"], outs["history2"])
    assert 0 < d_hd and d_hist < 1.5 * d_int8 + 1e-3
    assert not torch.equal(second_after_first, outs["history"])
    assert torch.equal(second_after_first, second_after_first2)
    assert not _same(h_a, h_b)      # the history is in use at step 1 ...
    assert _same(h_c, h_b)          # ... and another image's tokens do not meet it


# ---- 4b. the VAE at sizes whose mid block is not a multiple of 64 pixels ---------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(96, 160), (80, 112)])
def test_encoder_at_sizes_that_were_refused(setup, H, W):
    s = setup
    assert ((H // 8) * (W // 8)) % 64 != 0
    _, u8 = _image(H, W, H + W)
    got = s["enc"].encode_moments(u8.cuda())
    again = s["enc"].encode_moments(u8.cuda())
    torch.cuda.synchronize()
    ref = encode_ref(s["sd_enc"], s["vcfg"], preprocess_u8(u8))
    rel = _rel_rmse(nhwc_moments_to_nchw(got.cpu(), H // 8, W // 8), ref)
    print(f"encoder {H}x{W} (mid block {(H // 8) * (W // 8)} pixels): moments rel-RMSE {rel:.4f}")
    assert got.shape == ((H // 8) * (W // 8), 32) and torch.isfinite(got.float()).all()
    assert _same(got, again)
    assert rel < 3e-2


def test_decoder_at_a_size_that_was_refused(setup):
    s = setup
    h, w = 12, 20
    packed = (torch.randn(1, (h // 2) * (w // 2), 64, generator=torch.Generator().manual_seed(5)) * 0.8).bfloat16()
    ref_img, ref_u8 = V.latents_to_image(s["sd_dec"], s["vcfg"], packed, h, w)
    img = s["dec"].decode_packed(packed[0].cuda(), h, w, output_type="pt")
    u8 = s["dec"].decode_packed(packed[0].cuda(), h, w, output_type="np")
    torch.cuda.synchronize()
    rel = _rel_rmse(img, ref_img[0])
    px = float(((u8.float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"decoder latent {h}x{w} (240 mid-block pixels): image rel-RMSE {rel:.4f}, pixel RMSE {px:.5f}")
    assert img.shape == (3, 8 * h, 8 * w)
    assert rel < 3e-2 and px < 1e-2


@pytest.mark.parametrize("rows,cols", [(7, 64), (33, 240), (5, 140), (3, 4096), (2, 16356)])
def test_softmax_rows_strided(hip, rows, cols):
    """stride == columns: the bits of td_softmax_rows_f32_bf16; with a pad: the valid columns equal the unpadded call's bits, the pad
    columns exactly zero whatever the score buffer holds there."""
    L = hip.lib()
    g = torch.Generator().manual_seed(rows + cols)
    sc = (torch.randn(rows, cols, generator=g) * 4).cuda()
    scale = 0.0442
    base = torch.empty(rows, cols, dtype=BF, device="cuda")
    hip.check(L.td_softmax_rows_f32_bf16(hip.ptr(sc), hip.ptr(base), rows, cols, ctypes.c_float(scale), hip.stream_ptr()))
    same = torch.full((rows, cols), 7.0, dtype=BF, device="cuda")
    hip.check(L.td_softmax_rows_strided_f32_bf16(hip.ptr(sc), hip.ptr(same), rows, cols, cols, ctypes.c_float(scale), hip.stream_ptr()))
    ld = (cols + 63) // 64 * 64 + (64 if cols % 64 == 0 else 0)
    padded = torch.full((rows, ld), float("nan"), device="cuda")      # the pad of the scores is never read
    padded[:, :cols] = sc
    out = torch.full((rows, ld), 7.0, dtype=BF, device="cuda")
    hip.check(L.td_softmax_rows_strided_f32_bf16(hip.ptr(padded), hip.ptr(out), rows, cols, ld, ctypes.c_float(scale), hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _same(same, base)
    assert _same(out[:, :cols], base)
    assert not (_i16(out[:, cols:]) != 0).any()
    want = torch.softmax(sc.float() * scale, dim=-1)
    assert float((base.float() - want).abs().max()) < 2.0 ** -8


# ---- 5. the CFG step kernel, bit-exact --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 3.5, 3.7, 7.25])
@pytest.mark.parametrize("n", [8, 64, 1000 * 8, 4096 * 64])
def test_cfg_step_bit_exact(hip, scale, n):
    """flux_cfg_step_ against the eager torch statements ON THE DEVICE: noise_pred = neg + s * (pos - neg) with s a Python float, then
    the scheduler step as td_euler_step_bf16's comment states it.  3.7 is not a bf16 number: it pins where the scalar is rounded."""
    g = torch.Generator().manual_seed(n + int(scale * 100))
    x = torch.randn(n, generator=g).bfloat16()
    pos = (torch.randn(n, generator=g) * 2).bfloat16()
    neg = (torch.randn(n, generator=g) * 2).bfloat16()
    k = n // 8
    neg[:k] = pos[:k]                                             # pos == neg lanes
    pos[k:k + 2], neg[k:k + 2] = torch.tensor([0.0, -0.0]).bfloat16(), torch.tensor([-0.0, 0.0]).bfloat16()
    if n >= 64:
        pos[-8:] = torch.tensor([3e37, -3e37, 1e30, 65504.0, 1e-30, -1e-38, 2.5e38, 1.0]).bfloat16()
        neg[-8:] = torch.tensor([1e37, 3e37, -1e30, -65504.0, -1e-30, 1e-38, 2.0e38, -1.0]).bfloat16()
    x, pos, neg = x.cuda(), pos.cuda(), neg.cuda()
    dt = -0.0371                                                  # not a bf16 number
    sig = torch.tensor([0.9371, 0.9], dtype=torch.float32, device="cuda")
    dt_t = sig[1] - sig[0]
    noise_pred = neg + scale * (pos - neg)
    want = (x.to(torch.float32) + dt_t * noise_pred).to(noise_pred.dtype)
    got = x.clone()
    _ops().flux_cfg_step_(got, pos, neg, scale, float(dt_t))
    torch.cuda.synchronize()
    fin = torch.isfinite(want.float())
    bad = int((_i16(got)[fin] != _i16(want)[fin]).sum())
    print(f"cfg step n {n} scale {scale}: {bad} of {int(fin.sum())} finite lanes differ from eager torch on the device")
    assert bad == 0
    assert torch.equal(torch.isfinite(got.float()), fin)
    assert abs(float(dt_t) - dt) < 1e-6


def test_cfg_step_refusals(hip):
    x = torch.zeros(72, dtype=BF, device="cuda")
    a, b = torch.zeros(72, dtype=BF, device="cuda"), torch.zeros(72, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _ops().flux_cfg_step_(x[:12].clone(), a[:12].clone(), b[:12].clone(), 3.5, -0.1)
    with pytest.raises(RuntimeError, match="16-byte"):
        _ops().flux_cfg_step_(x[4:68], a[:64], b[:64], 3.5, -0.1)
    with pytest.raises(RuntimeError, match="overlap"):
        _ops().flux_cfg_step_(x[:64], x[8:72], b[:64], 3.5, -0.1)
    with pytest.raises(RuntimeError, match="contiguous elements"):
        _ops().flux_cfg_step_(x[:64], a[:56], b[:64], 3.5, -0.1)


# ---- 6. the CFG loop -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ref", [False, True])
def test_denoise_cfg(setup, with_ref):
    s = setup
    cfg, sd, pos = s["cfg"], s["sd"], s["tr"]
    neg = pos.fork()
    h2 = w2 = 8
    S, Sr, T, n, scale = 64, 96, 24, 4, 3.5
    lat, ref, pe, pool = _inputs(cfg, S, Sr, T, seed=31)
    npe, npool = s["npe"][0].cpu(), s["npool"][0].cpu()
    ids, rid = R.latent_image_ids(h2, w2), reference_ids(8, 12)
    sig = _prepare(pos, pe, pool, ids, n, S)
    _prepare(neg, npe, npool, ids, n, S)
    if with_ref:
        pos.set_reference_tokens(ref.cuda(), rid)
        neg.set_reference_tokens(ref.cuda(), rid)
    # the Python composition
    xC = lat.cuda().clone()
    for i in range(n):
        vp, vn = pos.forward_step(xC, i).clone(), neg.forward_step(xC, i).clone()
        _ops().flux_cfg_step_(xC, vp, vn, scale, float(sig[i + 1] - sig[i]))
    xA = lat.cuda().clone()
    pos.denoise_cfg(neg, xA, sig, scale)
    xP = lat.cuda().clone()
    pos.denoise(xP, sig)
    torch.cuda.synchronize()
    want = denoise_ref(sd, cfg, lat[None], ref[None] if with_ref else None, rid, pe[None], pool[None], h2, w2, n,
                       neg=(npe[None], npool[None]), scale=scale)
    d = _rel_rmse(xA[None], want)
    print(f"4-step CFG denoise (reference tokens: {with_ref}): ~oracle {d:.4f}; CFG moves the plain run by {_rel_rmse(xA, xP):.4f}")
    assert _same(xA, xC)
    assert d < 2e-2
    assert not _same(xA, xP)
    # mismatched contexts are refused
    _prepare(neg, npe, npool, R.latent_image_ids(4, 4), n, 16)
    with pytest.raises(RuntimeError):
        pos.denoise_cfg(neg, lat.cuda().clone(), sig, scale)
    _prepare(neg, npe, npool, ids, 2, S)
    if with_ref:
        neg.set_reference_tokens(ref.cuda(), rid)      # (set_condition voided them)
    with pytest.raises(RuntimeError, match="timesteps"):
        pos.denoise_cfg(neg, lat.cuda().clone(), sig, scale)
    with pytest.raises(RuntimeError, match="same"):
        pos.denoise_cfg(pos, lat.cuda().clone(), sig, scale)
    _prepare(neg, npe, npool, ids, n, S)                       # reference tokens on one context only
    pos.set_reference_tokens(ref.cuda(), rid)
    with pytest.raises(RuntimeError, match="96 / 0 reference tokens"):
        pos.denoise_cfg(neg, lat.cuda().clone(), sig, scale)
    with pytest.raises(ValueError, match="ref_ids"):
        pos.set_reference_tokens(ref.cuda())


# ---- 7. the pipeline against the CPU loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hr,Wr", [(96, 160), (128, 192)])
@pytest.mark.parametrize("cfg_on", [False, True])
def test_pipeline_matches_cpu_loop(setup, Hr, Wr, cfg_on):
    """128 x 128 out, 4 steps; the reference 96 x 160 has a 240-pixel mid block (the padded attention), 128 x 192 a 384-pixel one (the
    unpadded path): a failure says which half is at fault."""
    s = setup
    N = 4
    img, u8 = _image(Hr, Wr, Hr)
    kw = _kw(s, image=img)
    if cfg_on:
        kw.update(negative_prompt_embeds=s["npe"], negative_pooled_prompt_embeds=s["npool"], true_cfg_scale=3.5)
    out = s["pipe"](generator=_gen(7), output_type="latent", **kw).images
    px = s["pipe"](generator=_gen(7), output_type="np", **kw).images
    noise = torch.randn((1, 16, 16, 16), generator=_gen(7), device="cuda", dtype=BF).cpu()
    mom = encode_ref(s["sd_enc"], s["vcfg"], preprocess_u8(u8))
    ref = latents_ref(mom, None, None, 0.0, SCALING, SHIFT)
    neg = (s["npe"].cpu(), s["npool"].cpu()) if cfg_on else None
    x = denoise_ref(s["sd"], s["cfg"], R.pack_latents(noise), ref, reference_ids(Hr // 16, Wr // 16), s["pe"][:1].cpu(), s["pool"][:1].cpu(), 8, 8, N,
                    3.5, neg=neg, scale=3.5)
    _, ref_u8 = V.latents_to_image(s["sd_dec"], s["vcfg"], x, 16, 16)
    rel = _rel_rmse(out[0], x[0])
    prmse = float(((px[0].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"kontext 128x128, reference {Hr}x{Wr}, CFG {cfg_on}, {N} steps: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}")
    assert out.shape == (1, 64, LAT)
    assert rel < 2e-2 and prmse < 1e-2


@pytest.mark.parametrize("case", ["default", "latents", "cfg"])
def test_generator_position_after_a_call(setup, case):
    """Only the noise [B, 16, h, w] is drawn (the reference latents are the posterior's mode); nothing with latents=."""
    s = setup
    img, _ = _image(96, 160, 9)
    g, r = _gen(13), _gen(13)
    kw = _kw(s, image=img, output_type="latent")
    draws = 1
    if case == "latents":
        kw["latents"], draws = torch.zeros(1, 64, LAT, dtype=BF, device="cuda"), 0
    if case == "cfg":
        kw.update(negative_prompt_embeds=s["npe"], negative_pooled_prompt_embeds=s["npool"], true_cfg_scale=2.0)
    s["pipe"](generator=g, **kw)
    after = torch.randn(64, generator=g, device="cuda", dtype=BF)
    for _ in range(draws):
        torch.randn((1, 16, 16, 16), generator=r, device="cuda", dtype=BF)
    want = torch.randn(64, generator=r, device="cuda", dtype=BF)
    assert _same(after, want)


def test_pipeline_hands_the_engine_what_the_spec_says(setup):
    """A 16-channel tensor image is used as it is: the bits of the hand-driven engine with ids (1, y, x); ids with first column 0 give other
    bits.  image=None gives FluxPipelineRewritePrompt's bits.  The caller's latents are not written."""
    s = setup
    tr = s["tr"]
    lat = torch.randn(1, 64, LAT, generator=torch.Generator().manual_seed(2)).to(BF).cuda()
    keep = lat.clone()
    il = torch.randn(1, 16, 12, 20, generator=torch.Generator().manual_seed(4)).to(BF).cuda()
    kw = _kw(s, latents=lat, output_type="latent")
    a = s["pipe"](image=il, **kw).images
    assert _same(lat, keep)
    packed = R.pack_latents(il)[0].contiguous()
    rid = reference_ids(6, 10)
    outs = []
    for first in (1, 0):
        ids = rid.clone()
        ids[:, 0] = first
        sig = _prepare(tr, s["pe"][0], s["pool"][0], R.latent_image_ids(8, 8), 4, 64)
        tr.set_reference_tokens(packed, ids)
        x = lat[0].clone()
        tr.denoise(x, sig)
        outs.append(x)
    torch.cuda.synchronize()
    assert _same(a[0], outs[0]) and not _same(a[0], outs[1])
    # image=None: plain text-to-image on the same loop
    b = s["pipe"](image=None, generator=_gen(3), **_kw(s, output_type="latent")).images
    c = s["t2i"](prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=128, width=128, num_inference_steps=4, guidance_scale=3.5,
                 generator=_gen(3), output_type="latent").images
    assert _same(b, c)


def test_pil_output_auto_resize_warning_and_capacity(setup):
    s = setup
    img, _ = _image(100, 170, 3)                       # _auto_resize=False: floored to 96 x 160
    out = s["pipe"](image=img, generator=_gen(1), **_kw(s))
    im = out.images[0]
    assert im.size == (128, 128) and im.mode == "RGB"
    # the capacity refusal names both numbers (64 latent + 448 reference + ... here: a 256 x 256 reference = 256 tokens; capacity 512 holds it;
    # a transformer with 256 does not)
    from thinkdiff.models import FluxKontextPipelineRewritePrompt
    small = build_engine(s["cfg"], s["sd"], max_img_tokens=256)
    p = FluxKontextPipelineRewritePrompt(transformer=small, vae=s["dec"], vae_encoder=s["enc"])
    with pytest.raises(ValueError, match=r"64 latent \+ 256 reference tokens = 320 exceeds the transformer's capacity 256"):
        p(image=_image(256, 256, 4)[0], **_kw(s))
    # true_cfg_scale > 1 without a negative prompt: a warning and the plain loop's bits
    with pytest.warns(UserWarning, match="not enabled"):
        a = s["pipe"](image=img, generator=_gen(2), true_cfg_scale=4.0, **_kw(s, output_type="latent")).images
    b = s["pipe"](image=img, generator=_gen(2), **_kw(s, output_type="latent")).images
    assert _same(a, b)
