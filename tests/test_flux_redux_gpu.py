"""FLUX.1 Redux on the GPU (restatements: tests/redux_common.py).

Tolerances:
  * td_redux_compose_bf16 against `compose_ref`, and the pipeline against `redux_pipeline_ref` fed the tower's and the prior's own bf16 outputs:
    bit for bit (torch.equal) -- one rounding contract, no summation freedom.
  * tiny tower against transformers' fp32 SiglipVisionModel: relative RMSE < 2e-2, the bar tests/test_vision_towers_gpu.py holds the other towers to.
  * released widths (2 layers) and the prior: e_hip < 1.5 e_ref + 2e-3, e_ref = torch bf16 on the CPU against fp32 on the CPU (that file's full-size form).
  * end to end against oracle/flux_ref.py: relative RMSE < 2e-2, the bar of tests/test_flux_engine_gpu.py::test_denoise_loop_matches_oracle.
"""
import pytest
import torch

import redux_common as C

pytestmark = pytest.mark.gpu


def _scales(B):
    g = torch.Generator().manual_seed(B)
    return (C.SCALES + [float(v) for v in torch.randn(12, generator=g)])[:B]


@pytest.mark.parametrize("D", [8, 768, 4096, 4104])
def test_compose_kernel_equals_the_restatement(hip, D):
    import thinkdiff.ops  # noqa: F401  (registers torch.ops.thinkdiff_hip)
    for B in (1, 2, 3, 16):
        sc = _scales(B)
        for T, S in ((1, 0), (0, 1), (1, 1), (5, 7), (37, 29)):
            text = C.spread_inputs((B, T, D), seed=10 * B + T) if T else None
            image = C.spread_inputs((B, S, D), seed=10 * B + S + 1) if S else None
            dev = lambda t: t.cuda() if t is not None else None
            got = hip.redux_compose(dev(text), dev(image), sc)
            assert got.shape == (T + S, D) and torch.equal(got.cpu(), C.compose_ref(text, image, sc)), (B, T, S)
            if T and S:
                # text = NULL: T rows of +0.0 (bit pattern 0), nothing read
                got = hip.redux_compose(None, dev(image), sc, T=T)
                assert torch.equal(got.cpu(), C.compose_ref(None, image, sc, T=T)) and not got[:T].view(torch.int16).any(), (B, T, S)
                # text_bstride = 0: one text stream shared by every b, still added B times
                got = hip.redux_compose(dev(text[:1]), dev(image), sc)
                assert torch.equal(got.cpu(), C.compose_ref(text[:1], image, sc)), (B, T, S)
                got = torch.ops.thinkdiff_hip.redux_compose(dev(text), dev(image), sc, 0)
                assert torch.equal(got.cpu(), C.compose_ref(text, image, sc)), (B, T, S)
    torch.cuda.synchronize()


def test_compose_kernel_identity_sentinels_and_op(hip):
    import thinkdiff.ops  # noqa: F401
    D, T, S = 4096, 5, 7
    text, image = C.spread_inputs((1, T, D), seed=1), C.spread_inputs((1, S, D), seed=2)
    text[0, 0, :4] = torch.tensor([-0.0, 0.0, float("inf"), -1e-30])
    got = hip.redux_compose(text.cuda(), image.cuda(), [1.0])
    assert torch.equal(got.cpu().view(torch.int16), torch.cat([text[0], image[0]]).view(torch.int16))          # B = 1, scale 1: the inputs' bits
    # ldo = D + 16: the columns beyond D keep the sentinel
    x3 = C.spread_inputs((3, T + S, D), seed=3)
    buf = torch.full((T + S, D + 16), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.redux_compose(x3[:, :T].contiguous().cuda(), x3[:, T:].contiguous().cuda(), C.SCALES[:3], out=buf[:, :D])
    assert torch.equal(buf[:, :D].cpu(), C.compose_ref(None, x3, C.SCALES[:3])) and bool((buf[:, D:] == 7.0).all())
    # the pooled form (T = 1, S = 0, D = 768), with and without a source; the torch op against the ctypes call
    pooled = C.spread_inputs((2, 1, 768), seed=4)
    a = hip.redux_compose(pooled.cuda(), None, [1.0, 0.5])
    b = torch.ops.thinkdiff_hip.redux_compose(pooled.cuda(), None, [1.0, 0.5], 0)
    assert a.shape == (1, 768) and torch.equal(a, b) and torch.equal(a.cpu(), C.compose_ref(pooled, None, [1.0, 0.5]))
    z = hip.redux_compose(None, None, [1.0, 0.5], T=1, D=768, device=torch.device("cuda", torch.cuda.current_device()))
    assert z.shape == (1, 768) and not z.view(torch.int16).any()
    zi = torch.ops.thinkdiff_hip.redux_compose(None, image.cuda(), [0.37], T)
    assert torch.equal(zi.cpu(), C.compose_ref(None, image, [0.37], T=T))
    with pytest.raises(RuntimeError):
        torch.ops.thinkdiff_hip.redux_compose(text.cuda(), image.cuda(), [1.0] * 17, 0)


@pytest.fixture(scope="module")
def tiny(hip):
    """(config, transformers fp32 tower, HIP tower) of the tiny config: 2 heads of 72, MLP 304, image 42 -> 9 patches."""
    from thinkdiff.models.vision_towers import HipSiglipVisionModel
    cfg, ref = C.tiny_siglip(seed=0)
    return cfg, ref, HipSiglipVisionModel(C.vision_sd(ref), num_heads=cfg.num_attention_heads, eps=cfg.layer_norm_eps)


def test_tiny_tower_matches_transformers(hip, tiny):
    cfg, ref, tower = tiny
    pix = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(1))
    want = C.siglip_hidden_ref(ref, pix)
    got = tower(pix).last_hidden_state
    torch.cuda.synchronize()
    moved = C.rel_rmse(C.siglip_hidden_ref(ref, pix, layers=False), want)
    e = C.rel_rmse(got, want)
    print(f"tiny SigLIP tower rel-RMSE vs fp32 transformers {e:.4f}; without the layers the reference moves by {moved:.3f}")
    assert moved > 0.3                                                     # the encoder layers are not a no-op
    assert got.shape == (2, 9, 144) and got.dtype == torch.bfloat16 and e < 2e-2
    with pytest.raises(hip.ThinkDiffHipError, match=r"16 patches.*holds 9"):
        tower(torch.zeros(1, 3, 56, 56))


def test_released_widths_two_layers(hip):
    from thinkdiff.models.vision_towers import HipSiglipVisionModel
    cfg, ref = C.tiny_siglip(seed=3, hidden_size=1152, intermediate_size=4304, num_attention_heads=16, image_size=384)
    pix = torch.randn(1, 3, 384, 384, generator=torch.Generator().manual_seed(2)).bfloat16()
    exact = C.siglip_hidden_ref(ref, pix.float())
    tower = HipSiglipVisionModel(C.vision_sd(ref), num_heads=16, eps=cfg.layer_norm_eps)
    assert tower.layers[0]["fc1_w"].shape == (4352, 1152) and tower.patch_w.shape == (1152, 640)
    got = tower(pix).last_hidden_state
    torch.cuda.synchronize()
    want16 = C.siglip_hidden_ref(ref.bfloat16(), pix)
    e_hip, e_ref = C.rel_rmse(got, exact), C.rel_rmse(want16, exact)
    print(f"so400m widths, 2 layers, 729 tokens: HIP vs exact {e_hip:.4f}, torch bf16 vs exact {e_ref:.4f}")
    assert got.shape == (1, 729, 1152) and bool(torch.isfinite(got.float()).all())
    assert e_hip < 1.5 * e_ref + 2e-3


def test_prior_matches_torch(hip):
    from thinkdiff.models.flux_redux import ReduxImageEncoder
    g = torch.Generator().manual_seed(5)
    rn = lambda std, *s: (torch.randn(*s, generator=g) * std).bfloat16()
    sd = {"redux_up.weight": rn(0.03, 3 * 4096, 1152), "redux_up.bias": rn(0.05, 3 * 4096), "redux_down.weight": rn(0.01, 4096, 3 * 4096),
          "redux_down.bias": rn(0.05, 4096)}
    x = rn(1.0, 1, 729, 1152)
    F = torch.nn.functional

    def torch_prior(dtype):
        w = {k: v.to(dtype) for k, v in sd.items()}
        return F.linear(F.silu(F.linear(x.to(dtype), w["redux_up.weight"], w["redux_up.bias"])), w["redux_down.weight"], w["redux_down.bias"])

    exact, want16 = torch_prior(torch.float32), torch_prior(torch.bfloat16)
    enc = ReduxImageEncoder(sd)
    got = enc(x.cuda()).image_embeds
    torch.cuda.synchronize()
    e_hip, e_ref = C.rel_rmse(got, exact), C.rel_rmse(want16, exact)
    print(f"ReduxImageEncoder (1152 -> 12288 -> 4096), 729 rows: HIP vs exact {e_hip:.4f}, torch bf16 vs exact {e_ref:.4f}")
    assert (enc.redux_dim, enc.txt_in_features) == (1152, 4096) and got.shape == (1, 729, 4096)
    assert e_hip < 1.5 * e_ref + 2e-3


@pytest.fixture(scope="module")
def prior_pipe(hip, tiny):
    """The pipeline over the tiny tower and a random prior whose output width is the tiny FLUX config's joint width (512)."""
    from thinkdiff.models import FluxPriorReduxPipelineRewritePrompt, ReduxImageEncoder
    from thinkdiff.models.flux_redux import ReduxDefaultImageProcessor
    _cfg, _ref, tower = tiny
    return FluxPriorReduxPipelineRewritePrompt(tower, ReduxDefaultImageProcessor(size=42), ReduxImageEncoder.from_random(144, 512, seed=4))


def _own_embeds(pipe, pix):
    return pipe.image_embedder(pipe.image_encoder(pix).last_hidden_state).image_embeds


def test_pipeline_composition_is_bit_exact(hip, prior_pipe):
    g = torch.Generator().manual_seed(6)
    pix = torch.randn(2, 3, 42, 42, generator=g)
    emb = _own_embeds(prior_pipe, pix)
    assert emb.shape == (2, 9, 512)
    pe1, pool1 = torch.randn(1, 12, 512, generator=g).bfloat16(), torch.randn(1, 256, generator=g).bfloat16()
    pe2, pool2 = torch.randn(2, 12, 512, generator=g).bfloat16(), torch.randn(2, 256, generator=g).bfloat16()
    cases = [
        (pix[:1], dict(max_sequence_length=16), (1, 25, 512), (1, 768)),                                  # one image, no text: 16 zero rows
        (pix, dict(max_sequence_length=16, prompt_embeds_scale=[0.7, 0.3], pooled_prompt_embeds_scale=[1.0, 0.5]), (1, 25, 512), (1, 768)),
        (pix, dict(prompt_embeds=pe1, pooled_prompt_embeds=pool1, prompt_embeds_scale=[0.7, 0.3]), (1, 21, 512), (1, 256)),      # one text, two images
        (pix, dict(prompt_embeds=pe2, pooled_prompt_embeds=pool2, prompt_embeds_scale=[0.7, 0.3], pooled_prompt_embeds_scale=0.5), (1, 21, 512), (1, 256)),
    ]
    for px, kw, shape, pshape in cases:
        out = prior_pipe(px, **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
        want_pe, want_pool = C.redux_pipeline_ref(emb[:px.shape[0]], **kw)
        assert sorted(out.keys()) == ["pooled_prompt_embeds", "prompt_embeds"]
        assert out["prompt_embeds"].shape == shape and out["pooled_prompt_embeds"].shape == pshape
        assert torch.equal(out["prompt_embeds"].cpu(), want_pe) and torch.equal(out["pooled_prompt_embeds"].cpu(), want_pool), kw.keys()
        assert torch.equal(out.prompt_embeds, out["prompt_embeds"])
    tup = prior_pipe(pix[:1], max_sequence_length=16, return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 2 and tup[0].shape == (1, 25, 512)
    # a PIL image goes through the feature extractor; a tensor is taken as its output
    img = C.random_image(50, 70, seed=7)
    pv = prior_pipe.feature_extractor.preprocess(images=[img]).pixel_values
    assert torch.equal(pv, C.reference_processor(size={"height": 42, "width": 42}).preprocess(images=[img], return_tensors="pt").pixel_values)
    a, b = prior_pipe(img, max_sequence_length=16), prior_pipe([img], max_sequence_length=16)
    c = prior_pipe(pv, max_sequence_length=16)
    assert torch.equal(a["prompt_embeds"], c["prompt_embeds"]) and torch.equal(b["prompt_embeds"], c["prompt_embeds"])
    torch.cuda.synchronize()


def test_end_to_end_against_the_oracle(hip, prior_pipe):
    """`flux_pipe(**prior(image))` on the tiny FLUX config of tests/test_flux_engine_gpu.py::test_denoise_loop_matches_oracle (2 + 2 blocks, 16 x 16
    latent tokens, 4 steps) -- with pooled_projection_dim 768, the width of the prior's dummy pooled vector -- against oracle/flux_ref.py fed the same
    embeds, at that test's bar (relative RMSE < 2e-2)."""
    from oracle import flux_ref as R
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    from thinkdiff.models.flux_transformer import FluxTransformerConfig
    cfg = R.tiny_config(num_layers=2, num_single_layers=2, pooled_projection_dim=768)
    T = 16 + 9
    pipe = FluxPipelineRewritePrompt.from_random(FluxTransformerConfig(
        in_channels=cfg.in_channels, num_layers=2, num_single_layers=2, num_attention_heads=cfg.num_attention_heads, joint_attention_dim=cfg.joint_attention_dim,
        pooled_projection_dim=768, guidance_embeds=cfg.guidance_embeds), seed=7, with_vae=False, max_img_tokens=256, max_txt_tokens=64, max_steps=8)      # max_txt_tokens >= T
    sd = R.init_weights(cfg, seed=7)          # the oracle's own draw (norm weights near 1: the conditioning matters), as that test loads it
    pipe.transformer.load_state_dict(sd)
    g = torch.Generator().manual_seed(3)
    pix = torch.randn(1, 3, 42, 42, generator=g)
    lat = torch.randn(1, 16 * 16, 64, generator=g).bfloat16()
    run = lambda embeds: pipe(**embeds, height=256, width=256, num_inference_steps=4, guidance_scale=3.5, latents=lat.cuda(), output_type="latent").images
    embeds = prior_pipe(pix, max_sequence_length=16)
    assert embeds["prompt_embeds"].shape == (1, T, 512) and bool(embeds["prompt_embeds"][0, 16:].any())
    out = run(embeds)
    ref = R.denoise(sd, cfg, lat, embeds["prompt_embeds"].cpu(), embeds["pooled_prompt_embeds"].cpu(), 16, 16, 4, guidance_scale=3.5)
    e = C.rel_rmse(out, ref)
    print(f"flux_pipe(**prior(image)), 4 steps: rel-RMSE vs the bf16 oracle {e:.4f}")
    assert out.shape == ref.shape and e < 2e-2
    zero = prior_pipe(pix, max_sequence_length=16, prompt_embeds_scale=0.0)
    assert not bool((zero["prompt_embeds"] != 0).any()) and not bool((zero["pooled_prompt_embeds"] != 0).any())
    out0 = run(zero)
    torch.cuda.synchronize()
    print(f"image tokens at scale 1 against scale 0: the latents move by {C.rel_rmse(out, out0):.4f}")
    assert bool(torch.isfinite(out0.float()).all()) and not torch.equal(out, out0)          # the image tokens reach the latents
