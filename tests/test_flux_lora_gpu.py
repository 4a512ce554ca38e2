"""FLUX LoRA adapters on the GPU: the merge kernel against fp64, the engine's adapter registry against the CPU restatement (lora_common.py:
oracle/flux_ref.py on `merged_state_dict`) and against the path the engine already had (a plain engine loaded with the effective weights),
and the pipelines' loaders.  Tiny transformers (oracle/flux_ref.tiny_config, 1 + 1 blocks), the full FLUX.1 VAE architecture with seeded weights.

Bars that are tolerances are the project's own, as in test_flux_kontext_gpu.py: forward / denoise vs the bf16 oracle rel-RMSE < 2e-2, vs the
fp32 oracle < 1.5 e_ref + 2e-3 (e_ref: the bf16 oracle's own distance from the fp32 oracle), int8 vs the int8 oracle < 2e-2, fp8 vs the fp8
oracle < 3e-2, pixel RMSE < 1e-2.  Every parity check is preceded by the same comparison between the oracle WITH and WITHOUT the adapters,
which must be at least 3 x the bar: a pass cannot come from adapters that were never applied."""
import pytest
import torch
import torch.nn.functional as F

from kontext_common import build_engine, denoise_ref, reference_ids
from lora_common import block_linears, forward_ref, make_lora, merged_state_dict, rel_rmse
from oracle import flux_ref as R
from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, preprocess_u8

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SCALING, SHIFT = 0.3611, 0.1159
B_STD = 0.1
# The decoded image of these tiny models moves less than the velocity does: at b_std 0.1 the oracle's images with and without the adapter are
# 0.009 pixel RMSE apart (measured on the CPU), below the 1e-2 bar itself, at 0.4 they are 0.055 - 0.074 apart.  The pipeline tests therefore
# use an adapter of their own with b_std 0.5, and assert the 3 x separation on the oracle before grading anything.
B_STD_IMAGE = 0.5
EXTRA = ["x_embedder", "context_embedder", "transformer_blocks.0.norm1.linear", "proj_out"]


def _ops():
    from thinkdiff.ops import register
    return register()


def _i16(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_i16(a), _i16(b))


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- 1. the kernel against fp64 ------------------------------------------------------------------------------------------------------------
def _kernel_case(N, K, ranks, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    A = [(torch.randn(r, K, generator=g) / K ** 0.5).bfloat16() for r in ranks]
    B = [(torch.randn(N, r, generator=g) * 0.1).bfloat16() for r in ranks]
    return W.cuda(), [a.cuda() for a in A], [b.cuda() for b in B]


@pytest.mark.parametrize("scales", [(0.75, -1.5), (1.0, 1.0)])
@pytest.mark.parametrize("N,K,ranks", [(512, 512, [16]), (2048, 512, [4]), (3072, 3072, [64]), (3072, 3072, [128, 16]), (3072, 15360, [32]),
                                       (3072, 64, [8]), (512, 512, [5])])
def test_merge_kernel_vs_fp64(hip, N, K, ranks, scales):
    """Against ref = W + sum_i s_i B_i A_i in fp64 (on the device, torch's fp64 matmul):
    (a) every element: |out - ref| <= e + 2^-8 max(|ref|, |out|), e = (sum R + 3) 2^-24 (|W| + sum |s_i| |B_i| |A_i|) -- the textbook bound of an
        fp32 sum of sum R + 2 terms plus half a bf16 spacing;
    (b) the share of elements that are not RNE_bf16(ref) is <= 2e-4 (the same formula in CPU fp32 leaves 0 .. 6.6e-5 on these cases; a kernel
        that rounds the update to bf16 before adding it leaves 0.13 .. 0.29)."""
    W, A, B = _kernel_case(N, K, ranks, seed=N + K + sum(ranks))
    sc = list(scales[:len(ranks)])
    out = _ops().lora_merge(W, A, B, sc)
    torch.cuda.synchronize()
    ref = W.double()
    mag = W.double().abs()
    for a, b, s in zip(A, B, sc):
        ref = ref + s * (b.double() @ a.double())
        mag = mag + abs(s) * (b.double().abs() @ a.double().abs())
    e = (sum(ranks) + 3) * 2.0 ** -24 * mag
    o = out.double()
    slack = e + 2.0 ** -8 * torch.maximum(ref.abs(), o.abs()) - (o - ref).abs()
    n_bad = int((slack < 0).sum())
    share = float((_i16(out) != _i16(ref.float().bfloat16())).double().mean())
    print(f"lora_merge [{N}, {K}] ranks {ranks} scales {sc}: bound violations {n_bad} (worst slack {float(slack.min()):.3e}), not RNE(ref): {share:.2e}")
    assert out.shape == (N, K) and out.dtype == BF
    assert n_bad == 0
    assert share <= 2e-4


def test_merge_kernel_identities(hip):
    W, A, B = _kernel_case(3072, 3072, [128, 16], seed=1)
    W[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-38, -1e-38], dtype=BF, device="cuda")
    # all scales 0: the base bits (signed zeros included)
    assert _same(_ops().lora_merge(W, A, B, [0.0, 0.0]), W)
    assert _same(_ops().lora_merge(W, [], [], []), W)
    # in place == out of place, bit for bit
    out = _ops().lora_merge(W, A, B, [0.75, -1.5])
    w2 = W.clone()
    back = _ops().lora_merge_(w2, A, B, [0.75, -1.5])
    assert back.data_ptr() == w2.data_ptr() and _same(w2, out) and not _same(out, W)
    # a pair at scale 0 beside an active one contributes nothing
    assert _same(_ops().lora_merge(W, A, B, [0.75, 0.0]), _ops().lora_merge(W, A[:1], B[:1], [0.75]))
    # N % 32 != 0: the partial last row band leaves its neighbours alone
    Wp, Ap, Bp = _kernel_case(72, 128, [16], seed=2)
    buf = torch.full((80, 128), 7.0, dtype=BF, device="cuda")
    buf[:72] = Wp
    _ops().lora_merge_(buf[:72], Ap, Bp, [1.0])
    assert _same(buf[:72], _ops().lora_merge(Wp, Ap, Bp, [1.0])) and bool((buf[72:] == 7.0).all())
    with pytest.raises(RuntimeError, match="K=40"):
        _ops().lora_merge(torch.zeros(8, 40, dtype=BF, device="cuda"), [torch.zeros(4, 40, dtype=BF, device="cuda")],
                          [torch.zeros(8, 4, dtype=BF, device="cuda")], [1.0])
    with pytest.raises(RuntimeError, match="do not fit"):
        _ops().lora_merge(W, [A[0][:, :64].contiguous()], B[:1], [1.0])
    with pytest.raises(RuntimeError, match="at most 8"):
        _ops().lora_merge(W, A[:1] * 9, B[:1] * 9, [1.0] * 9)


@pytest.mark.parametrize("N,K,ranks", [(96, 192, [24]), (72, 128, [40, 3]), (32, 64, [1])])
def test_merge_kernel_exact_integers(hip, N, K, ranks):
    """Small-integer W, A, B (asymmetric: every row, column and rank index has its own pattern) whose result is an integer of magnitude
    <= 256: exact in every step, so the output must EQUAL the reference -- a transposed or k-permuted fragment map cannot pass."""
    g = torch.Generator().manual_seed(N + K)
    W = torch.randint(-40, 41, (N, K), generator=g).float()
    A = [torch.randint(-1, 3, (r, K), generator=g).float() for r in ranks]
    B = [torch.randint(-2, 2, (N, r), generator=g).float() for r in ranks]
    sc = [1.0, -1.0][:len(ranks)]
    ref = W.clone()
    for a, b, s in zip(A, B, sc):
        ref += s * (b @ a)
    assert float(ref.abs().max()) <= 256 and not torch.equal(ref, W)
    out = _ops().lora_merge(W.bfloat16().cuda(), [a.bfloat16().cuda() for a in A], [b.bfloat16().cuda() for b in B], sc)
    torch.cuda.synchronize()
    bad = int((out.float().cpu() != ref).sum())
    print(f"exact-integer merge [{N}, {K}] ranks {ranks}: {bad} of {N * K} elements differ")
    assert bad == 0


# ---- the engine fixture ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg = R.tiny_config(num_layers=1, num_single_layers=1)
    sd = R.init_weights(cfg, seed=4)
    mods = block_linears(cfg)
    l1 = make_lora(cfg, mods, 16, seed=1, b_std=B_STD)
    # the second adapter overlaps the first on six Linears and reaches the embedders, an adaLN Linear and the final projection
    l2 = make_lora(cfg, mods[3:9] + EXTRA, 8, seed=2, b_std=B_STD, alpha=12.0)
    lp = make_lora(cfg, mods, 16, seed=3, b_std=B_STD_IMAGE)
    g = torch.Generator().manual_seed(21)
    h2 = w2 = 8
    return dict(cfg=cfg, sd=sd, tr=build_engine(cfg, sd), l1=l1, l2=l2, lp=lp, h2=h2, w2=w2,
                lat=torch.randn(h2 * w2, 64, generator=g).bfloat16(), pe=torch.randn(24, cfg.joint_attention_dim, generator=g).bfloat16(),
                pool=torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16())


def _prepare(m, s, n=2):
    from thinkdiff.models.flux_transformer import effective_scalar
    sig = R.make_sigmas(n, s["lat"].shape[0])
    m.set_condition(s["pe"].cuda(), s["pool"].cuda(), R.latent_image_ids(s["h2"], s["w2"]))
    m.set_timesteps([effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]], float((torch.tensor([3.5]).bfloat16() * 1000).float()))
    return sig


def _forward(m, s, n=2):
    _prepare(m, s, n)
    out = m.forward_step(s["lat"].cuda(), 0).clone()
    torch.cuda.synchronize()
    return out


def _oracle(s, sd, dtype=BF):
    return forward_ref(sd, s["cfg"], s["lat"], s["pe"], s["pool"], s["h2"], s["w2"], dtype=dtype)[0]


# ---- 2. + 3. discrimination, then parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one", "two"])
def test_forward_and_denoise_parity(setup, case):
    s = setup
    cfg, sd, m = s["cfg"], s["sd"], s["tr"]
    loras, weights = ([s["l1"]], [1.0]) if case == "one" else ([s["l1"], s["l2"]], [0.7, -0.4])
    merged16 = merged_state_dict(sd, loras, weights, BF)
    merged32 = merged_state_dict(sd, loras, weights, torch.float32)
    ref16, ref32, base16 = _oracle(s, merged16), _oracle(s, merged32, torch.float32), _oracle(s, sd)
    sep, e_ref = rel_rmse(base16, ref16), rel_rmse(ref16, ref32)
    n = 4
    lat1, pe1, pool1 = s["lat"][None], s["pe"][None], s["pool"][None]
    den16 = R.denoise(merged16, cfg, lat1, pe1, pool1, s["h2"], s["w2"], n)[0]
    den_base = R.denoise(sd, cfg, lat1, pe1, pool1, s["h2"], s["w2"], n)[0]
    sep_den = rel_rmse(den_base, den16)
    print(f"[{case}] oracle with vs without the adapters: velocity {sep:.4f}, 4-step denoise {sep_den:.4f}; bf16 ~ fp32 oracle {e_ref:.4f}")
    assert sep >= 3 * 2e-2, "the fixture does not discriminate: raise b_std"      # on the oracle, before anything is graded
    try:
        m.load_lora_adapter(loras[0], "first")
        if case == "two":
            m.load_lora_adapter(loras[1], "second")
            m.set_adapters(["first", "second"], weights)
        assert m.active_adapters() == dict(zip(["first", "second"], map(float, weights)))
        info = m.lora_info()
        assert info["adapters"] == len(loras) and info["params_touched"] == (17 if case == "one" else 21) and info["bytes_held"] > 0
        out = _forward(m, s)
        sig = _prepare(m, s, n)
        x = s["lat"].cuda().clone()
        m.denoise(x, sig)
        torch.cuda.synchronize()
    finally:
        m.unload_lora()
    e16, e32, d16 = rel_rmse(out, ref16), rel_rmse(out, ref32), rel_rmse(x, den16)
    print(f"[{case}] hip ~ bf16 oracle {e16:.4f}  hip ~ fp32 oracle {e32:.4f}  4-step denoise ~ bf16 oracle {d16:.4f}")
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3
    assert d16 < 2e-2


# ---- 4. bits against the path the engine already had ------------------------------------------------------------------------------------
def _fresh_with(s, params):
    m = build_engine(s["cfg"], s["sd"])
    m.load_state_dict(params)
    return m


@pytest.mark.parametrize("precision", ["int8", "fp8"])
def test_effective_weights_in_a_plain_engine_give_the_same_bits(setup, precision):
    s = setup
    sd, m = s["sd"], s["tr"]
    oracle_flag = "INT8_BLOCK_LINEARS" if precision == "int8" else "FP8_BLOCK_LINEARS"
    merged16 = merged_state_dict(sd, [s["l1"], s["l2"]], [0.7, -0.4], BF)
    setattr(R, oracle_flag, True)
    try:
        ref8 = _oracle(s, merged16)
    finally:
        setattr(R, oracle_flag, False)
    try:
        m.load_lora_adapter(s["l1"], "first")
        m.load_lora_adapter(s["l2"], "second")
        m.set_adapters(["first", "second"], [0.7, -0.4])
        eff = m.state_dict()
        assert sorted(eff) == sorted(sd) and all(eff[k].shape == sd[k].shape for k in sd)
        changed = sorted(k for k in sd if not _same(eff[k].cpu(), sd[k]))
        assert len(changed) == 21 and all(k.endswith(".weight") for k in changed)
        plain = _fresh_with(s, eff)
        assert plain.lora_info() == {"adapters": 0, "params_touched": 0, "bytes_held": 0}
        a16, p16 = _forward(m, s), _forward(plain, s)
        # adapters attached BEFORE the precision is set
        m.set_precision(precision)
        plain.set_precision(precision)
        a8, p8 = _forward(m, s), _forward(plain, s)
        # ... and AFTER: back to no adapters in the 8-bit mode, then attach again
        m.unload_lora()
        base8 = _forward(m, s)
        m.load_lora_adapter(s["l1"], "first")
        m.load_lora_adapter(s["l2"], "second")
        m.set_adapters(["first", "second"], [0.7, -0.4])
        b8 = _forward(m, s)
    finally:
        m.unload_lora()
        m.set_precision("bf16")
    e8 = rel_rmse(a8, ref8)
    print(f"{precision}: adapted engine ~ {precision} oracle on the merged dict {e8:.4f}; the adapters move the {precision} velocity by {rel_rmse(base8, a8):.4f}")
    assert _same(a16, p16)
    assert _same(a8, p8) and _same(b8, p8)
    assert not _same(base8, a8) and not _same(a8, a16)
    assert e8 < (2e-2 if precision == "int8" else 3e-2)


# ---- 5. purity ---------------------------------------------------------------------------------------------------------------------------
def test_the_merge_is_a_pure_function(setup):
    s = setup
    sd, m = s["sd"], s["tr"]
    base_out = _forward(m, s)
    try:
        m.load_lora_adapter(s["l1"], "first")
        m.load_lora_adapter(s["l2"], "second")
        assert m.active_adapters() == {"first": 1.0, "second": 1.0}      # loading activates at 1.0 beside those already active
        name = "transformer_blocks.0.attn.add_q_proj.weight"               # both adapters touch it
        m.set_adapters(["first", "second"], [0.7, -0.4])
        wA, outA = m.read_param(name), _forward(m, s)
        m.set_adapters(["first", "second"], [0.7, -0.4])
        assert _same(m.read_param(name), wA) and _same(_forward(m, s), outA)
        m.set_adapters(["second"], [1.3])
        wB = m.read_param(name)
        m.set_adapters(["first", "second"], [0.7, -0.4])
        assert not _same(wB, wA) and _same(m.read_param(name), wA) and _same(_forward(m, s), outA)
        # against the restatement, parameter by parameter: at most the last bit, and that rarely
        merged16 = merged_state_dict(sd, [s["l1"], s["l2"]], [0.7, -0.4], BF)
        eff = m.state_dict()
        off = sum(int((_i16(eff[k].cpu()) != _i16(merged16[k])).sum()) for k in sd)
        total = sum(v.numel() for k, v in sd.items() if not _same(merged16[k], v))
        print(f"effective weights vs the fp64 restatement: {off} of {total} adapted elements differ in bits")
        assert off <= 2e-4 * total
        # weights all 0, and the empty set: base bits
        m.set_adapters(["first", "second"], [0.0, 0.0])
        assert all(_same(m.read_param(k).cpu(), v) for k, v in sd.items()) and _same(_forward(m, s), base_out)
        m.set_adapters([])
        assert m.active_adapters() == {} and _same(_forward(m, s), base_out)
        # delete one == an engine that only ever loaded the other
        m.set_adapters(["first", "second"], [0.7, -0.4])
        m.delete_adapters("first")
        assert m.list_adapters() == ["second"] and m.lora_info()["params_touched"] == 10
        other = build_engine(s["cfg"], sd)
        other.load_lora_adapter(s["l2"], "second")
        other.set_adapters(["second"], [-0.4])
        assert all(_same(m.read_param(k), other.read_param(k)) for k in sd) and _same(_forward(m, s), _forward(other, s))
        with pytest.raises(ValueError, match="unknown adapter 'first'"):
            m.set_adapters(["first"])
        with pytest.raises(RuntimeError, match="unknown adapter 'nope'"):
            _ops().flux_lora_set_adapters(int(m._h.value), ["nope"], [1.0])
        with pytest.raises(RuntimeError, match="already holds a pair"):
            a = torch.zeros(4, 512, dtype=BF, device="cuda")
            _ops().flux_lora_load(int(m._h.value), "second", name, a, torch.zeros(512, 4, dtype=BF, device="cuda"), 1.0)
        for bad, match in (("transformer_blocks.0.attn.norm_q.weight", "not the weight of a Linear"), ("proj_out.bias", "not the weight of a Linear"),
                           ("no.such.weight", "unknown parameter")):
            with pytest.raises(RuntimeError, match=match):
                _ops().flux_lora_load(int(m._h.value), "x", bad, torch.zeros(4, 64, dtype=BF, device="cuda"), torch.zeros(64, 4, dtype=BF, device="cuda"), 1.0)
    finally:
        m.unload_lora()
    assert m.lora_info() == {"adapters": 0, "params_touched": 0, "bytes_held": 0}
    assert all(_same(m.read_param(k).cpu(), v) for k, v in sd.items())
    assert _same(_forward(m, s), base_out)


# ---- 6. forks and staleness --------------------------------------------------------------------------------------------------------------
def test_forks_and_stale_contexts(setup):
    s = setup
    m = s["tr"]
    fork = m.fork()
    lat = s["lat"].cuda()
    try:
        _prepare(m, s)
        _prepare(fork, s)
        before = m.forward_step(lat, 0).clone()
        m.load_lora_adapter(s["l1"], "first")
        for ctx in (m, fork):      # prepared before the adapters were set: the precomputed embeddings and modulations are stale
            with pytest.raises(RuntimeError, match="weights changed since td_flux_set_condition / td_flux_set_timesteps"):
                ctx.forward_step(lat, 0)
            with pytest.raises(RuntimeError, match="weights changed since"):
                ctx.denoise(lat.clone(), R.make_sigmas(2, 64))
        a, b = _forward(m, s), _forward(fork, s)
        assert _same(a, b) and not _same(a, before)
        with pytest.raises(RuntimeError, match="parent"):
            fork.load_lora_adapter(s["l2"], "second")
        with pytest.raises(RuntimeError, match="clear the adapters first"):
            m.load_state_dict({"transformer_blocks.0.attn.to_q.weight": s["sd"]["transformer_blocks.0.attn.to_q.weight"]}, strict=False)
        with pytest.raises(RuntimeError, match="clear the adapters first"):
            m.init_random(1)
        m.load_state_dict({"proj_out.weight": s["sd"]["proj_out.weight"]}, strict=False)      # not adapted: as ever
    finally:
        m.unload_lora()
    m.load_state_dict(s["sd"])
    assert _same(_forward(m, s), before) and _same(_forward(fork, s), before)


# ---- 7. pipelines ------------------------------------------------------------------------------------------------------------------------
def _image(n, seed):
    from PIL import Image
    u8 = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    u8 = F.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return Image.fromarray(u8.numpy()), u8


def _pixels(img):
    """VaeImageProcessor.denormalize of a decoded image: [0, 1]."""
    return (img.float().cpu() / 2 + 0.5).clamp(0, 1)


def _px_rmse(a, b):
    return float((_pixels(a) - _pixels(b)).pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def pipes(setup):
    from thinkdiff.models import FluxImg2ImgPipelineRewritePrompt, FluxKontextPipelineRewritePrompt, FluxPipelineRewritePrompt
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder, AutoencoderKLEncoder
    s = setup
    vcfg = V.VaeConfig()
    sd_dec, sd_enc = V.init_weights(vcfg, seed=12), encoder_init_weights(vcfg, seed=13)
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(32, 32))
    dec.load_state_dict(sd_dec)
    enc = AutoencoderKLEncoder(AutoencoderKLConfig(), max_image_size=(256, 256))
    enc.load_state_dict(sd_enc)
    tr = s["tr"]
    t2i = FluxPipelineRewritePrompt(transformer=tr, vae=dec)
    return dict(vcfg=vcfg, sd_dec=sd_dec, sd_enc=sd_enc, t2i=t2i, i2i=FluxImg2ImgPipelineRewritePrompt.from_pipe(t2i, enc),
                kontext=FluxKontextPipelineRewritePrompt(transformer=tr, vae=dec, vae_encoder=enc))


def test_text_to_image_pipeline_with_a_lora_file(setup, pipes, tmp_path):
    from safetensors.torch import save_file
    s, p = setup, pipes
    cfg, sd, pipe = s["cfg"], s["sd"], p["t2i"]
    fn = str(tmp_path / "adapter.safetensors")
    save_file(s["lp"], fn)
    N = 4
    pe, pool = s["pe"][None].cuda(), s["pool"][None].cuda()
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pool, height=128, width=128, num_inference_steps=N, guidance_scale=3.5, output_type="pt")
    noise = torch.randn((1, 16, 16, 16), generator=_gen(7), device="cuda", dtype=BF).cpu()

    def oracle_image(weights):
        merged = merged_state_dict(sd, [s["lp"]], weights, BF) if weights else sd
        x = R.denoise(merged, cfg, R.pack_latents(noise), s["pe"][None], s["pool"][None], 8, 8, N)
        return V.latents_to_image(p["sd_dec"], p["vcfg"], x, 16, 16)[0][0]
    ref_lora, ref_half, ref_base = oracle_image([1.0]), oracle_image([0.5]), oracle_image(None)
    sep = _px_rmse(ref_base, ref_lora)
    print(f"oracle image with vs without the adapter: pixel RMSE {sep:.4f} (weight 0.5: {_px_rmse(ref_base, ref_half):.4f})")
    assert sep >= 3 * 1e-2, "the fixture does not discriminate: raise b_std"
    try:
        base = pipe(generator=_gen(7), **kw).images[0]
        name = pipe.load_lora_weights(fn)
        assert pipe.get_active_adapters() == [name] and pipe.get_list_adapters() == {"transformer": [name]}
        full = pipe(generator=_gen(7), **kw).images[0]
        with pytest.raises(NotImplementedError, match="set_adapters"):
            pipe(generator=_gen(7), joint_attention_kwargs={"scale": 0.5}, **kw)
        pipe.set_adapters([name], [0.5])
        half = pipe(generator=_gen(7), **kw).images[0]
        pipe.set_adapters([name], [1.0])
        pipe.fuse_lora(lora_scale=0.5)
        fused = pipe(generator=_gen(7), **kw).images[0]
        pipe.unfuse_lora()
        unfused = pipe(generator=_gen(7), **kw).images[0]
        pipe.unload_lora_weights()
        after = pipe(generator=_gen(7), **kw).images[0]
        assert pipe.get_active_adapters() == []
        pipe(generator=_gen(7), joint_attention_kwargs={"scale": 0.5}, **kw)      # no adapters: swallowed as ever
        # a directory + weight_name, with an explicit adapter name and alpha
        other = pipe.load_lora_weights(str(tmp_path), weight_name="adapter.safetensors", adapter_name="style", alpha=8)
        half_by_alpha = pipe(generator=_gen(7), **kw).images[0]
    finally:
        pipe.unload_lora_weights()
    torch.cuda.synchronize()
    d_full, d_half, d_base, d_after = _px_rmse(full, ref_lora), _px_rmse(half, ref_half), _px_rmse(base, ref_base), _px_rmse(after, ref_base)
    print(f"t2i 128x128, {N} steps: pixel RMSE vs the oracle: adapter {d_full:.5f}, weight 0.5 {d_half:.5f}, none {d_base:.5f}; "
          f"adapter image vs the oracle WITHOUT the adapter {_px_rmse(full, ref_base):.4f}")
    assert d_full < 1e-2 and d_half < 1e-2 and d_base < 1e-2 and d_after < 1e-2
    assert _px_rmse(full, ref_base) >= 3 * 1e-2
    assert other == "style" and _same(after, base) and _same(fused, half) and _same(unfused, full) and _same(half_by_alpha, half)


def test_img2img_and_kontext_pipelines_with_an_adapter(setup, pipes):
    from thinkdiff.models.flux_img2img import get_timesteps
    s, p = setup, pipes
    cfg, sd = s["cfg"], s["sd"]
    merged = merged_state_dict(sd, [s["lp"]], [1.0], BF)
    pe, pool = s["pe"][None], s["pool"][None]
    N, n = 8, 128
    img, u8 = _image(n, 2)
    mom = encode_ref(p["sd_enc"], p["vcfg"], preprocess_u8(u8))

    def img2img_ref(weights_sd):
        g = _gen(7)
        eps = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
        noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
        t_start = get_timesteps(N, 0.6)
        sig = R.make_sigmas(N, 64)
        x = latents_ref(mom, eps, noise, float(sig[t_start]), SCALING, SHIFT)
        sig_t = torch.from_numpy(sig)
        for i in range(t_start, N):
            t = (sig_t[i] * 1000.0).expand(1).bfloat16()
            v = R.transformer_forward(weights_sd, cfg, x, pe, pool, t / 1000, R.latent_image_ids(8, 8).bfloat16(), torch.zeros(pe.shape[1], 3).bfloat16(),
                                      torch.full([1], 3.5))
            x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
        return V.latents_to_image(p["sd_dec"], p["vcfg"], x, 16, 16)[0][0]

    def kontext_ref(weights_sd):
        noise = torch.randn((1, 16, 16, 16), generator=_gen(7), device="cuda", dtype=BF).cpu()
        ref = latents_ref(mom, None, None, 0.0, SCALING, SHIFT)
        x = denoise_ref(weights_sd, cfg, R.pack_latents(noise), ref, reference_ids(8, 8), pe, pool, 8, 8, 4, 3.5)
        return V.latents_to_image(p["sd_dec"], p["vcfg"], x, 16, 16)[0][0]
    kw = dict(prompt_embeds=pe.cuda(), pooled_prompt_embeds=pool.cuda(), height=n, width=n, guidance_scale=3.5, output_type="pt")
    try:
        p["i2i"].load_lora_weights(s["lp"], adapter_name="a")      # a dict; the three pipelines share the transformer, hence the adapter
        assert p["kontext"].get_active_adapters() == ["a"]
        got_i2i = p["i2i"](image=img, strength=0.6, num_inference_steps=N, generator=_gen(7), **kw).images[0]
        got_k = p["kontext"](image=img, num_inference_steps=4, generator=_gen(7), max_area=n * n, _auto_resize=False, **kw).images[0]
        with pytest.raises(NotImplementedError, match="set_adapters"):
            p["i2i"](image=img, strength=0.6, num_inference_steps=N, generator=_gen(7), joint_attention_kwargs={"scale": 2.0}, **kw)
    finally:
        p["kontext"].unload_lora_weights()
    torch.cuda.synchronize()
    for name, got, ref_fn in (("img2img", got_i2i, img2img_ref), ("kontext", got_k, kontext_ref)):
        with_lora, without = ref_fn(merged), ref_fn(sd)
        d, sep = _px_rmse(got, with_lora), _px_rmse(without, with_lora)
        print(f"{name} with the adapter: pixel RMSE vs its restatement on the merged dict {d:.5f}; the restatement with vs without the adapter {sep:.4f}")
        assert d < 1e-2
        assert sep >= 3 * 1e-2, "the fixture does not discriminate: raise b_std"
