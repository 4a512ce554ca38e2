"""GPU tests of the first-block cache: the two kernels against fp64, and the engine against the test-local restatement (block_cache_common.py) on
the tiny fixture (3 + 3 layers, 16 x 16 latent tokens, 40 text tokens, 8 steps).

Tolerances, stated once:
  * velocities / latents vs the bf16 restatement: relative RMSE <= 2e-2, and vs the float64 restatement no further than 1.5 x the bf16 restatement
    itself is (+ 2e-3) -- the rule of test_flux_engine_gpu.py;
  * a logged metric vs the float64 restatement's: |hip - f64| <= 1.5 x |bf16 - f64| + 0.02 x metric -- relative to the reference's own deviation,
    because the metric is a ratio of two sums over a bf16 residual and moves by per cent between two correct bf16 pipelines;
  * the kernels' sums vs fp64: relative error <= 1e-5; r and tail bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import block_cache_common as C
from oracle import flux_ref as R

pytestmark = pytest.mark.gpu

LOOP_SCHEDULE = "CsCssCsC"


def _ops():
    import thinkdiff.ops  # noqa: F401
    return torch.ops.thinkdiff_hip


@pytest.fixture(scope="module")
def fx(hip):
    cfg, sd, lat, pe, pool = C.fixture()
    sd64, (lat64, pe64, pool64) = C.widen(sd, lat, pe, pool)
    sch = C.parse_schedule(LOOP_SCHEDULE)
    x16, s16 = C.denoise(sd, cfg, lat, pe, pool, C.H2, C.W2, C.N_STEPS, schedule=sch)
    x64, s64 = C.denoise(sd64, cfg, lat64, pe64, pool64, C.H2, C.W2, C.N_STEPS, schedule=sch)
    return dict(cfg=cfg, sd=sd, lat=lat, pe=pe, pool=pool, sd64=sd64, lat64=lat64, pe64=pe64, pool64=pool64, m=C.build_engine(cfg, sd),
                loop16=(x16, s16), loop64=(x64, s64))


@pytest.fixture
def eng(fx):
    """The module's engine, prepared for the 8-step loop, cache off before and after."""
    m = fx["m"]
    m.disable_cache()
    fx["sig"] = C.prepare(m, fx["pe"], fx["pool"], C.N_STEPS)
    yield m
    m.disable_cache()
    m.set_precision("bf16")
    m.set_attention("bf16")
    m.set_reference_tokens(None)


def _metric_bar(hip, m16, m64, what):
    for i in range(1, len(hip)):
        bar = 1.5 * abs(m16[i] - m64[i]) + 0.02 * m64[i]
        print(f"{what} forward {i}: metric hip {hip[i]:.5f}  bf16 restatement {m16[i]:.5f}  f64 restatement {m64[i]:.5f}  bar {bar:.5f}")
    for i in range(1, len(hip)):
        assert abs(hip[i] - m64[i]) <= 1.5 * abs(m16[i] - m64[i]) + 0.02 * m64[i], (what, i)


# ---- 1. kernels vs fp64 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,lds,prev", [(257, 512, (640, 512, 576), True), (33, 3072, None, True), (1, 8, None, True), (33, 3072, None, False),
                                             (4096, 3072, None, True)])
def test_kernels_match_fp64_and_repeat_bit_for_bit(hip, rows, D, lds, prev):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(rows + D)
    ld1, ld0, ldp = lds or (D, D, D)
    view = lambda ld, scale: (scale * torch.randn(rows, ld, generator=g, device="cuda")).bfloat16()[:, :D]
    h0 = view(ld0, 1.0)
    h1 = (h0.float() + view(ld1, 0.3).float()).bfloat16() if ld1 == ld0 else view(ld1, 1.0)
    want_r = (h1.float() - h0.float()).bfloat16()
    # r_prev near r, as between two denoise steps (and far from it in the strided case): both sums are sums of many small terms
    rp = ((want_r.float() + view(ldp, 0.05).float()).bfloat16() if ldp == D else view(ldp, 1.0)) if prev else None
    if rp is not None and ldp != D:
        assert rp.stride(0) == ldp
    r, sums = ops.block_cache_head(h1, h0, rp)
    r2, sums2 = ops.block_cache_head(h1, h0, rp)
    torch.cuda.synchronize()
    assert r.shape == (rows, D) and torch.equal(r, want_r) and torch.equal(r2, r)
    assert sums.dtype == torch.float64 and torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    if prev:
        want = torch.stack([(want_r.double() - rp.double()).abs().sum(), rp.double().abs().sum()])
        rel = ((sums - want).abs() / want).tolist()
        print(f"[{rows} x {D}] sums {sums.tolist()}  fp64 {want.tolist()}  relative error {rel}")
        assert max(rel) <= 1e-5
    else:
        assert sums.tolist() == [0.0, 0.0]
    tail = ops.block_cache_tail(h1, h0)
    assert torch.equal(tail, want_r)
    if lds:      # a strided second operand, and the in-place form the engine uses
        assert torch.equal(ops.block_cache_tail(r, rp), (r.float() - rp.float()).bfloat16())
        from thinkdiff import _hip
        b = h0.clone()
        _hip.check(_hip.lib().td_block_cache_tail_bf16(_hip.ptr(h1), h1.stride(0), _hip.ptr(b), D, _hip.ptr(b), D, rows, D, _hip.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(b, want_r)


# ---- 2. off is off ----------------------------------------------------------------------------------------------------------------------------
def _traced(m, lat, step=0):
    m.trace_begin(400)
    v = m.forward_step(lat, step).clone()
    tr = m.trace_end()
    return v, sum(c["launches"] for c in tr.values())


def test_off_is_off(fx):
    cfg = fx["cfg"]
    m = C.build_engine(cfg, fx["sd"])      # an engine that has never seen the cache
    sig = C.prepare(m, fx["pe"], fx["pool"], C.N_STEPS)
    lat = fx["lat"][0].cuda().contiguous()
    v0, n0 = _traced(m, lat)
    x0 = lat.clone()
    m.denoise(x0, sig)
    # the plain bf16 forward: x_embedder, 8 launches per double block, 5 per single block, the final norm and proj_out
    assert n0 == 3 + 8 * cfg.num_layers + 5 * cfg.num_single_layers
    m.set_cache_schedule([1, 0])
    v_c, n_c = _traced(m, lat)
    v_s, n_s = _traced(m, lat)
    assert m.cache_stats()[1] == [True, False]
    assert torch.equal(v_c, v0) and n_c == n0 + 2                      # + the head (one record: both its kernels) and the tail
    assert not torch.equal(v_s, v0) and n_s == 1 + 8 + 2 + 2           # x_embedder, block 0, head + add, final norm + proj_out
    m.disable_cache()
    assert m.is_cache_enabled is False
    v1, n1 = _traced(m, lat)
    x1 = lat.clone()
    m.denoise(x1, sig)
    torch.cuda.synchronize()
    assert torch.equal(v1, v0) and n1 == n0 and torch.equal(x1, x0)
    assert m.cache_stats() == ([], [])


# ---- 3. always-compute is exact ---------------------------------------------------------------------------------------------------------------
def test_threshold_zero_computes_every_step_and_changes_no_bit(fx, eng):
    from thinkdiff.models import FirstBlockCacheConfig, apply_first_block_cache
    lat = fx["lat"][0].cuda().contiguous()
    x_off = lat.clone()
    eng.denoise(x_off, fx["sig"])
    apply_first_block_cache(eng, FirstBlockCacheConfig(threshold=0.0))
    assert eng.is_cache_enabled
    x_on = lat.clone()
    eng.denoise(x_on, fx["sig"])
    torch.cuda.synchronize()
    metrics, computed = eng.cache_stats()
    assert torch.equal(x_on, x_off)
    assert computed == [True] * C.N_STEPS and math.isinf(metrics[0]) and all(0 < v < 10 for v in metrics[1:])
    fx["metrics_all_computed"] = metrics


# ---- 4. a skipped forward, single forwards, no trajectory -------------------------------------------------------------------------------------
def _three_forwards(sd, cfg, dt, A, B, Cc, pe, pool):
    t, gd = C.scalars(dt, 0.7324)
    ii, ti = R.latent_image_ids(C.H2, C.W2).to(dt), torch.zeros(C.T_TXT, 3).to(dt)
    sch = [1, 1, 0]
    st = C.CacheState()
    C.forward(sd, cfg, st, A, pe, pool, t, ii, ti, gd, schedule=sch)
    tail_a = st.tail
    C.forward(sd, cfg, st, Cc, pe, pool, t, ii, ti, gd, schedule=sch)
    out = {}
    for name, use in (("ok", None), ("drop", "drop"), ("stale", tail_a)):
        s2 = C.CacheState()
        s2.r_prev, s2.tail, s2.count = st.r_prev, st.tail, st.count
        out[name] = C.forward(sd, cfg, s2, B, pe, pool, t, ii, ti, gd, schedule=sch, tail_use=use)
        assert s2.computed == [False]
    return out


def test_skipped_forward_adds_the_last_computed_tail(fx, eng):
    cfg, sd = fx["cfg"], fx["sd"]
    g = torch.Generator().manual_seed(11)
    A, B, Cc = [torch.randn(1, C.H2 * C.W2, 64, generator=g).bfloat16() for _ in range(3)]
    o16 = _three_forwards(sd, cfg, torch.bfloat16, A, B, Cc, fx["pe"], fx["pool"])
    o64 = _three_forwards(fx["sd64"], cfg, torch.float64, A.double(), B.double(), Cc.double(), fx["pe64"], fx["pool64"])
    eng.set_timesteps([float((torch.tensor([0.7324]).bfloat16() * 1000).float())], float((torch.tensor([3.5]).bfloat16() * 1000).float()))
    eng.set_cache_schedule([1, 1, 0])
    eng.forward_step(A[0].cuda().contiguous(), 0)
    eng.forward_step(Cc[0].cuda().contiguous(), 0)
    v = eng.forward_step(B[0].cuda().contiguous(), 0)[None].cpu()
    assert eng.cache_stats()[1] == [True, True, False]
    e16, e64, e_ref = C.rel_rmse(v, o16["ok"]), C.rel_rmse(v, o64["ok"]), C.rel_rmse(o16["ok"], o64["ok"])
    d_drop, d_stale = C.rel_rmse(o16["drop"], o16["ok"]), C.rel_rmse(o16["stale"], o16["ok"])
    print(f"skipped velocity: hip~bf16 {e16:.4f}  hip~f64 {e64:.4f}  bf16~f64 {e_ref:.4f};  tail dropped {d_drop:.4f}  A's tail {d_stale:.4f} from the right one")
    assert e16 <= 2e-2
    assert e64 <= 1.5 * e_ref + 2e-3
    assert d_drop >= 4 * e16 and d_stale >= 4 * e16


# ---- 5. the loop under a schedule -------------------------------------------------------------------------------------------------------------
def test_denoise_loop_under_a_schedule(fx, eng):
    (x16, s16), (x64, s64) = fx["loop16"], fx["loop64"]
    sch = C.parse_schedule(LOOP_SCHEDULE)
    assert s16.computed == [bool(c) for c in sch] == s64.computed
    eng.set_cache_schedule(sch)
    x = fx["lat"][0].cuda().contiguous().clone()
    eng.denoise(x, fx["sig"])
    torch.cuda.synchronize()
    metrics, computed = eng.cache_stats()
    e = C.rel_rmse(x[None], x16)
    print(f"schedule {LOOP_SCHEDULE}: final latents hip~bf16 restatement {e:.4f}  (bf16~f64 restatement {C.rel_rmse(x16, x64):.4f})")
    assert computed == [bool(c) for c in sch] and math.isinf(metrics[0])
    assert e <= 2e-2
    _metric_bar(metrics, s16.metrics, s64.metrics, "loop")


# ---- 6. threshold mode is self-consistent -----------------------------------------------------------------------------------------------------
def test_threshold_mode_follows_its_own_metrics(fx, eng):
    from thinkdiff.models import FirstBlockCacheConfig
    lat = fx["lat"][0].cuda().contiguous()
    base = fx.get("metrics_all_computed")
    if base is None:
        eng.enable_cache(FirstBlockCacheConfig(threshold=0.0))
        eng.denoise(lat.clone(), fx["sig"])
        base = eng.cache_stats()[0]
    thr = float(np.float32(sorted(base[1:])[len(base[1:]) // 2]))      # inside the observed range: the median of the always-compute metrics
    eng.enable_cache(FirstBlockCacheConfig(threshold=thr))
    x = lat.clone()
    eng.denoise(x, fx["sig"])
    torch.cuda.synchronize()
    metrics, computed = eng.cache_stats()
    print(f"threshold {thr:.5f}: metrics {[round(v, 5) for v in metrics]}  decisions {''.join('C' if c else 's' for c in computed)}")
    assert len(metrics) == C.N_STEPS and computed[0] and math.isinf(metrics[0])
    for i in range(1, C.N_STEPS):
        assert computed[i] == (np.float32(metrics[i]) > np.float32(thr)), i
    assert any(computed[1:]) and not all(computed[1:])
    # r_prev advances on computed forwards only: the restatement replayed under the engine's own decisions logs the engine's metrics
    x16, s16 = C.denoise(fx["sd"], fx["cfg"], fx["lat"], fx["pe"], fx["pool"], C.H2, C.W2, C.N_STEPS, schedule=computed)
    x64, s64 = C.denoise(fx["sd64"], fx["cfg"], fx["lat64"], fx["pe64"], fx["pool64"], C.H2, C.W2, C.N_STEPS, schedule=computed)
    _metric_bar(metrics, s16.metrics, s64.metrics, "replay")
    assert C.rel_rmse(x[None], x16) <= 2e-2
    # a threshold nothing exceeds: one computed forward, then skips
    eng.enable_cache(FirstBlockCacheConfig(threshold=1e30))
    eng.denoise(lat.clone(), fx["sig"])
    assert eng.cache_stats()[1] == [True] + [False] * (C.N_STEPS - 1)


# ---- 7. images in flight ----------------------------------------------------------------------------------------------------------------------
def test_images_in_flight_decide_as_sequential_runs(fx, eng):
    from thinkdiff.models import FirstBlockCacheConfig, FluxTransformer2DModel
    g = torch.Generator().manual_seed(5)
    lat_b = torch.randn(C.H2 * C.W2, 64, generator=g).bfloat16().cuda()
    pe_b = torch.randn(1, C.T_TXT, fx["cfg"].joint_attention_dim, generator=g).bfloat16()
    pool_b = torch.randn(1, fx["cfg"].pooled_projection_dim, generator=g).bfloat16()
    lat_a = fx["lat"][0].cuda().contiguous()
    base = fx.get("metrics_all_computed") or [0.0, 0.4]
    eng.enable_cache(FirstBlockCacheConfig(threshold=float(sorted(base[1:])[len(base[1:]) // 2])))
    m2 = eng.fork()
    C.prepare(m2, pe_b, pool_b, C.N_STEPS)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    xa, xb = lat_a.clone(), lat_b.clone()
    FluxTransformer2DModel.denoise_multi([eng, m2], [xa, xb], fx["sig"], streams)
    torch.cuda.synchronize()
    logs = eng.cache_stats(), m2.cache_stats()
    ya, yb = lat_a.clone(), lat_b.clone()
    FluxTransformer2DModel.denoise_multi([eng], [ya], fx["sig"], streams[:1])
    torch.cuda.synchronize()
    FluxTransformer2DModel.denoise_multi([m2], [yb], fx["sig"], streams[1:])
    torch.cuda.synchronize()
    print("decisions in flight:", ["".join("C" if c else "s" for c in lg[1]) for lg in logs])
    assert torch.equal(xa, ya) and torch.equal(xb, yb)
    assert logs == (eng.cache_stats(), m2.cache_stats())
    assert not torch.equal(xa, xb) and logs[0][0] != logs[1][0]


# ---- 8. 8-bit history ---------------------------------------------------------------------------------------------------------------------------
def test_skipped_forward_voids_the_8bit_history(fx, eng):
    g = torch.Generator().manual_seed(13)
    xs = [torch.randn(C.H2 * C.W2, 64, generator=g).bfloat16().cuda() for _ in range(3)]
    eng.set_precision("int8", act_scales="history")
    eng.set_attention("fp8")
    out = {}
    for name, sch in (("CsC", [1, 0, 1]), ("CCC", [1, 1, 1])):
        eng.set_cache_schedule(sch)
        for i in range(3):
            v = eng.forward_step(xs[i], i).clone()
        out[name] = v
        assert eng.cache_stats()[1] == [bool(c) for c in sch]
    fresh = eng.fork()
    C.prepare(fresh, fx["pe"], fx["pool"], C.N_STEPS)
    want = fresh.forward_step(xs[2], 2).clone()      # no history: per-token scales measured on the spot, softmax references from the first tile
    torch.cuda.synchronize()
    assert torch.equal(out["CsC"], want)
    assert not torch.equal(out["CCC"], want)         # (with step 1 computed, step 2 does run on its history: the comparison above says something)


def test_pending_calibration_forces_a_computed_forward(fx, eng):
    g = torch.Generator().manual_seed(17)
    xs = [torch.randn(C.H2 * C.W2, 64, generator=g).bfloat16().cuda() for _ in range(3)]
    eng.set_precision("int8", act_scales="history", smoothing=True)
    eng.set_cache_schedule([1, 0, 0])
    eng.forward_step(xs[0], 0)                       # calibrates
    eng.set_precision("int8", act_scales="history", smoothing=True)      # the weights are quantised afresh: a calibration is pending again
    eng.forward_step(xs[1], 1)                       # the schedule says skip; the calibration must see every block
    eng.forward_step(xs[2], 2)
    torch.cuda.synchronize()
    assert eng.cache_stats()[1] == [True, True, False]


# ---- 9. composition and refusals ----------------------------------------------------------------------------------------------------------------
def test_true_cfg_keeps_two_logs(fx, eng):
    from thinkdiff.models import FirstBlockCacheConfig
    g = torch.Generator().manual_seed(19)
    pe_n = torch.randn(1, C.T_TXT, fx["cfg"].joint_attention_dim, generator=g).bfloat16()
    pool_n = torch.randn(1, fx["cfg"].pooled_projection_dim, generator=g).bfloat16()
    eng.enable_cache(FirstBlockCacheConfig(threshold=0.0))
    neg = eng.fork()
    C.prepare(neg, pe_n, pool_n, C.N_STEPS)
    x = fx["lat"][0].cuda().contiguous().clone()
    eng.denoise_cfg(neg, x, fx["sig"], 2.5)
    torch.cuda.synchronize()
    (mp, cp), (mn, cn) = eng.cache_stats(), neg.cache_stats()
    assert cp == cn == [True] * C.N_STEPS and math.isinf(mp[0]) and math.isinf(mn[0])
    assert all(a != b for a, b in zip(mp[1:], mn[1:]))
    # the loop resets both states at its start
    eng.denoise_cfg(neg, x, fx["sig"], 2.5)
    assert len(eng.cache_stats()[0]) == len(neg.cache_stats()[0]) == C.N_STEPS


def test_metric_covers_the_reference_rows(fx, eng):
    import kontext_common as K
    cfg = fx["cfg"]
    g = torch.Generator().manual_seed(23)
    A, B = [torch.randn(1, C.H2 * C.W2, 64, generator=g).bfloat16() for _ in range(2)]
    ref = torch.randn(1, 64, 64, generator=g).bfloat16()
    ref_ids = K.reference_ids(8, 8)
    logs, rs = {}, {}
    for dt, sd, pe, pool in ((torch.bfloat16, fx["sd"], fx["pe"], fx["pool"]), (torch.float64, fx["sd64"], fx["pe64"], fx["pool64"])):
        t, gd = C.scalars(dt, 0.7324)
        ii, ti = R.latent_image_ids(C.H2, C.W2).to(dt), torch.zeros(C.T_TXT, 3).to(dt)
        st = C.CacheState()
        C.forward(sd, cfg, st, A.to(dt), pe, pool, t, ii, ti, gd, schedule=[1, 1], ref=ref.to(dt), ref_ids=ref_ids)
        r_a = st.r_prev
        C.forward(sd, cfg, st, B.to(dt), pe, pool, t, ii, ti, gd, schedule=[1, 1], ref=ref.to(dt), ref_ids=ref_ids)
        logs[dt], rs[dt] = st.metrics, (r_a, st.r_prev)
    r_a, r_b = rs[torch.float64]
    S = C.H2 * C.W2
    assert r_a.shape[1] == S + 64
    latent_only = float((r_b[:, :S] - r_a[:, :S]).abs().sum() / r_a[:, :S].abs().sum())
    eng.set_timesteps([float((torch.tensor([0.7324]).bfloat16() * 1000).float())], float((torch.tensor([3.5]).bfloat16() * 1000).float()))
    eng.set_reference_tokens(ref[0].cuda(), ref_ids)
    eng.set_cache_schedule([1, 1])
    eng.forward_step(A[0].cuda().contiguous(), 0)
    eng.forward_step(B[0].cuda().contiguous(), 0)
    metrics = eng.cache_stats()[0]
    m16, m64 = logs[torch.bfloat16], logs[torch.float64]
    print(f"with 64 reference rows: metric hip {metrics[1]:.5f}  bf16 {m16[1]:.5f}  f64 {m64[1]:.5f};  over the latent rows alone {latent_only:.5f}")
    _metric_bar(metrics, m16, m64, "reference tokens")
    bar = 1.5 * abs(m16[1] - m64[1]) + 0.02 * m64[1]
    assert abs(latent_only - m64[1]) > 2 * bar, "the fixture does not tell the two row sets apart"
    assert abs(metrics[1] - latent_only) > bar


def test_refusals_name_their_cause(fx, eng):
    import controlnet_common as CN
    from thinkdiff import _hip
    L = _hip.lib()
    f32 = ctypes.c_float
    # a negative and a NaN threshold
    assert L.td_flux_set_block_cache(eng._h, 1, f32(-0.5)) == 2 and b"threshold -0.5" in L.td_last_error()
    assert L.td_flux_set_block_cache(eng._h, 1, f32(float("nan"))) == 2 and b"threshold nan" in L.td_last_error().lower()
    assert L.td_flux_set_block_cache(eng._h, 3, f32(0.1)) == 2 and b"mode 3" in L.td_last_error()
    # a schedule that starts with a skip
    with pytest.raises(_hip.ThinkDiffHipError, match="starts with a skip"):
        eng.set_cache_schedule([0, 1])
    assert not eng.is_cache_enabled
    # model-level setters on a fork
    fork = eng.fork()
    assert L.td_flux_set_block_cache(fork._h, 1, f32(0.1)) == 2 and b"fork" in L.td_last_error()
    assert L.td_flux_set_block_cache_schedule(fork._h, b"\x01\x00", 2) == 2 and b"fork" in L.td_last_error()
    with pytest.raises(_hip.ThinkDiffHipError, match="parent transformer"):
        fork.enable_cache()
    # a ControlNet model, and a forward with a ControlNet attached
    cfg_cn = R.tiny_config(num_layers=1, num_single_layers=0, guidance_embeds=False)
    cn = CN.build_controlnet(cfg_cn, CN.cn_init_weights(cfg_cn, seed=1), max_img_tokens=512, max_txt_tokens=64)
    with pytest.raises(_hip.ThinkDiffHipError, match="ControlNet model"):
        cn.enable_cache()
    lat = fx["lat"][0].cuda().contiguous()
    eng.attach_controlnet(cn)
    try:
        eng.enable_cache()
        with pytest.raises(RuntimeError, match="first-block cache is on .mode 1. and a ControlNet is attached"):
            eng.forward_step(lat, 0)
        with pytest.raises(RuntimeError, match="ControlNet is attached"):
            eng.denoise(lat.clone(), fx["sig"])
    finally:
        eng.attach_controlnet(None)
    v = eng.forward_step(lat, 0)                     # detached: the cache runs
    torch.cuda.synchronize()
    assert torch.isfinite(v.float()).all() and eng.cache_stats()[1][-1] is True
