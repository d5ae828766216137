"""Density control on the device (gs_density_accumulate / _decide / _plan / _restructure, gs_opacity_reset, gaussiansplat_amd.density):
bit for bit against the NumPy restatement of include/gsplat.h (tests/density_ref.py), the refusals, a frame on the restructured
renderer against a fresh renderer built from the new arrays, and a short training run with the 3DGS schedule."""
import math

import numpy as np
import pytest

import density_ref as D
from common import bits, dev, host, perturbed_start, refused, same_bits, synthetic_renderer

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = f32(-777.25)
PAD = 64                                    # rows of SENTINEL behind every destination: nothing may be written there


def _model(r):
    sd = r.splatData
    return [sd.means, sd.scales, sd.quaternions, sd.opacities, sd.shs]


def _frame(r, cam, dC):
    from gaussiansplat_amd import renderer as R
    R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
    R.resetGrads(r)
    R.backward(r, dC)


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize("deterministic", [False, True])
def test_accumulate_matches_the_reference_bit_for_bit(deterministic):
    import torch
    from gaussiansplat_amd import backend as B, synthetic
    from gaussiansplat_amd.density import DensityStats
    n, W, H, deg = 3000, 200, 136, 1                        # 12.5 x 8.5 tiles: ragged on both edges
    cams = [synthetic.scene_camera(W, view=v) for v in (0, 1)]
    scene = synthetic.make_scene(n, W, H, deg, seed=11)
    e = np.asarray(cams[0].eye, np.float64) + np.asarray(cams[1].eye, np.float64)
    out = np.arange(100, 112)                               # twelve gaussians moved out of both views
    scene["means"][out[0:3]] = (2.0 * e).astype(f32)         # behind both cameras
    scene["means"][out[3:6]] = (-3.0 * e).astype(f32)        # beyond `far`
    scene["means"][out[6:9]] = np.array([0.0, 40.0, 0.0], f32)   # in depth, far above the frame
    scene["means"][out[9:12], 1] = np.nan
    r = synthetic_renderer(n, deg, 0, W, H, scene=scene, export_debug=True, deterministic=deterministic, tile_parts=1)
    stats = DensityStats(r)
    ref = (np.zeros(n, f32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    for v, cam in enumerate(cams):
        _frame(r, cam, torch.as_tensor(synthetic.make_dC(W, H, 40 + v)).cuda())
        g2 = r.ctx.get_array(B.ARR_GRAD2D)
        vis, ext = D.visibility(*(r.ctx.get_array(a) for a in (B.ARR_BBS, B.ARR_TPS, B.ARR_RGB, B.ARR_SIG, B.ARR_MU, B.ARR_INVCOV)),
                                f32(cam.near), f32(cam.far))
        stats.accumulate()
        ref = D.accumulate(*ref, g2, W, H, vis, ext)
    twice = DensityStats(r)                                 # a second accumulate on the same frame doubles
    twice.accumulate(); twice.accumulate()
    one = D.accumulate(np.zeros(n, f32), np.zeros(n, np.int32), np.zeros(n, np.int32), g2, W, H, vis, ext)
    torch.cuda.synchronize()
    gs, cnt, mx = stats.grad_sum.cpu().numpy(), stats.count.cpu().numpy(), stats.max_extent.cpu().numpy()
    with np.errstate(invalid="ignore"):
        touched = float(np.mean(gs > 0))
    print("accumulate (deterministic=%d): %.1f %% of the gaussians have grad_sum > 0, %d visible in both views, largest extent %d px"
          % (deterministic, 100 * touched, int((cnt == 2).sum()), int(mx.max())))
    assert touched >= 0.30 and not cnt[out].any() and not mx[out].any()          # the conditions the comparison stands on
    assert same_bits(gs, ref[0], nan_equal=True), np.flatnonzero(bits(gs) != bits(ref[0]))[:8]
    assert np.array_equal(cnt, ref[1]) and np.array_equal(mx, ref[2])
    assert np.isnan(ref[0][out[9:12]]).all() or not ref[0][out[9:12]].any()      # (a NaN mean gives a NaN or a zero gradient, never a finite one)
    g2x, c2x, m2x = twice.grad_sum.cpu().numpy(), twice.count.cpu().numpy(), twice.max_extent.cpu().numpy()
    with np.errstate(invalid="ignore"):
        assert same_bits(g2x, one[0] + one[0], nan_equal=True) and same_bits(g2x, f32(2.0) * one[0], nan_equal=True)
    assert np.array_equal(c2x, 2 * one[1]) and np.array_equal(m2x, one[2])


# ---------------------------------------------------------------- decide (and its log_shrink reaching the children)
def test_decide_matches_the_reference_on_thresholds_and_nans():
    import torch
    from gaussiansplat_amd import backend as B, synthetic
    from gaussiansplat_amd.density import density_params
    n, deg = 2000, 1
    rng = np.random.default_rng(21)
    p = density_params(scene_extent=4.0, grad_threshold=2e-4, percent_dense=0.012, min_opacity=0.1, max_world_fraction=0.02, max_extent_px=20,
                       log_shrink=0.3)
    thr, lss, ls, mo, mw = (f32(x) for x in (p.grad_threshold, p.log_split_scale, p.log_shrink, p.min_opacity_logit, p.log_max_world_scale))
    px = p.max_extent_px
    scene = synthetic.make_scene(n, 128, 96, deg, seed=21)
    scene["scales"] = rng.uniform(-6.0, -2.0, (n, 3)).astype(f32)              # around log_split_scale (-3.04) and log_max_world_scale (-2.53)
    scene["opacities"] = rng.uniform(-4.0, 4.0, n).astype(f32)                 # around the opacity threshold (-2.2)
    cnt = rng.integers(0, 6, n).astype(np.int32)
    gs = (rng.random(n) * 4e-4).astype(f32) * cnt.astype(f32)                   # around grad_threshold * count
    ext = rng.integers(0, 40, n).astype(np.int32)
    # rows exactly on every threshold, one ulp to either side of the float ones, and NaN rows
    k = 0
    for c in (1, 3, 5):
        on = f32(thr * f32(c))
        for val in (on, np.nextafter(on, f32(0)), np.nextafter(on, f32(1))):
            cnt[k], gs[k], scene["opacities"][k], ext[k] = c, val, 0.0, 0; scene["scales"][k] = (-5.0, -4.0, -3.5); k += 1
    for centre in (lss, mw, f32(mw + ls)):                                     # the split scale, the world scale kept / after the shrink
        for val in (centre, np.nextafter(centre, f32(-10)), np.nextafter(centre, f32(10))):
            for dens in (0, 1):
                cnt[k], gs[k], scene["opacities"][k], ext[k] = 2, f32(dens), 0.0, 0; scene["scales"][k] = (-7.0, val, -6.5); k += 1
    for val in (mo, np.nextafter(mo, f32(-10)), np.nextafter(mo, f32(10))):
        cnt[k], gs[k], scene["opacities"][k], ext[k] = 2, 0.0, val, 0; scene["scales"][k] = (-5.0, -4.0, -3.5); k += 1
    for e in (19, 20, 21):
        cnt[k], gs[k], scene["opacities"][k], ext[k] = 2, 0.0, 0.0, e; scene["scales"][k] = (-5.0, -4.0, -3.5); k += 1
    gs[k] = np.nan; k += 1
    scene["scales"][k, 1] = np.nan; k += 1
    scene["scales"][k, 0] = np.nan; cnt[k], gs[k] = 2, 1.0; k += 1
    scene["opacities"][k] = np.nan; k += 1
    r = synthetic_renderer(n, deg, 0, scene=scene)
    t_gs, t_cnt, t_ext = dev(gs, None), dev(cnt, None), dev(ext, None)
    st = B.GsDensityStats(t_gs.data_ptr(), t_cnt.data_ptr(), t_ext.data_ptr())
    action = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    r._begin()
    r.ctx.density_decide(st, p, action.data_ptr())
    want = D.decide(scene["scales"], scene["opacities"], gs, cnt, ext, thr, lss, ls, mo, mw, px)
    got = action.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    c = D.counts(want)
    assert min(c) > 50, c                                                       # every class is well represented
    # the children of these split actions shrink by THIS decide's log_shrink
    assert r.ctx.density_plan(action.data_ptr()) == c
    noise = rng.standard_normal((n, 2, 3)).astype(f32)
    model = host(_model(r))
    new, _ = D.restructure(model, want, noise, log_shrink=ls)
    dst = [torch.full((D.n_out(c) + PAD, a.shape[1]), float(SENTINEL), device="cuda") for a in model]
    t_noise = dev(noise, None)
    r.ctx.density_restructure(action.data_ptr(), t_noise.data_ptr(), B.GsGrads(*[t.data_ptr() for t in dst]), [], [], D.n_out(c))
    for a, b in zip(host(dst), new):
        assert same_bits(a[:len(b)], b, nan_equal=True) and np.all(a[len(b):] == SENTINEL)
    # +Inf / 0 switch the world-scale and extent tests off; grad_threshold = +Inf switches densification off
    q = density_params(scene_extent=4.0, grad_threshold=math.inf, percent_dense=0.012, min_opacity=0.1, max_world_fraction=None, max_extent_px=0)
    r.ctx.density_decide(st, q, action.data_ptr())
    want = D.decide(scene["scales"], scene["opacities"], gs, cnt, ext, f32(np.inf), lss, f32(q.log_shrink), mo, f32(np.inf), 0)
    assert np.array_equal(action.cpu().numpy(), want) and set(np.unique(want)) == {0, 3}


# ---------------------------------------------------------------- restructure
def _actions(pattern, n, rng):
    if pattern == "mixed":
        return rng.choice(4, n, p=[0.5, 0.2, 0.15, 0.15]).astype(np.int32)
    return np.full(n, {"keep": 0, "prune": 3, "split": 2, "clone": 1}[pattern], np.int32)


def _restructure_case(r, n, deg, pattern, nsets, rng):
    import torch
    from gaussiansplat_amd import backend as B
    widths = [3, 3, 4, 1, 3 * (deg + 1) ** 2]
    model = host(_model(r))
    act = _actions(pattern, n, rng)
    c = D.counts(act)
    no = D.n_out(c)
    noise = rng.standard_normal((n, 2, 3)).astype(f32) if c[2] else None
    sets = [[rng.standard_normal((n, w)).astype(f32) for w in widths] for _ in range(nsets)]
    null = (1, 2) if nsets else None                                            # set 1 comes without its quaternion array
    ref_sets = [[None if null == (t, i) else a for i, a in enumerate(s)] for t, s in enumerate(sets)]
    new, new_sets = D.restructure(model, act, noise, sets=ref_sets)
    t_act = dev(act, None)
    t_noise = dev(noise, None) if noise is not None else None
    dst = [torch.full((no + PAD, w), float(SENTINEL), device="cuda") for w in widths]
    t_src = [[dev(a, None) for a in s] for s in sets]
    t_dst = [[torch.full((no + PAD, w), float(SENTINEL), device="cuda") for w in widths] for _ in range(nsets)]
    struct = lambda ts, t: B.GsGrads(*[None if null == (t, i) else x.data_ptr() for i, x in enumerate(ts)])
    r._begin()
    assert r.ctx.density_plan(t_act.data_ptr()) == c, (pattern, c)
    r.ctx.density_restructure(t_act.data_ptr(), t_noise.data_ptr() if t_noise is not None else None, B.GsGrads(*[t.data_ptr() for t in dst]),
                              [struct(s, t) for t, s in enumerate(t_src)], [struct(s, t) for t, s in enumerate(t_dst)], no)
    for k, (a, b) in enumerate(zip(host(dst), new)):
        assert same_bits(a[:no], b), (pattern, nsets, k, np.argwhere(bits(a[:no]) != bits(b))[:4])
        assert np.all(a[no:] == SENTINEL), (pattern, nsets, k)
    for t in range(nsets):
        for i, a in enumerate(host(t_dst[t])):
            if null == (t, i):
                assert np.all(a == SENTINEL)                                    # skipped: untouched
            else:
                assert same_bits(a[:no], new_sets[t][i]) and np.all(a[no:] == SENTINEL), (pattern, t, i)
    return c


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_restructure_matches_the_reference_bit_for_bit(n, deg):
    r = synthetic_renderer(n, deg, seed=30 + deg)
    rng = np.random.default_rng(1000 * deg + n)
    for pattern in ("mixed", "keep", "prune", "split", "clone"):
        for nsets in (0, 2):
            c = _restructure_case(r, n, deg, pattern, nsets, rng)
            assert sum((c[0], c[2], c[3])) == n
            if pattern == "prune":
                assert D.n_out(c) == 0
            if pattern == "split":
                assert D.n_out(c) == 2 * n


def test_restructure_more_than_1024_chunks():
    """300 001 gaussians are 1172 chunks of 256: a thread of the one scan workgroup sums two of them."""
    n, deg = 300_001, 3
    r = synthetic_renderer(n, deg, seed=33)
    c = _restructure_case(r, n, deg, "mixed", 2, np.random.default_rng(33))
    assert min(c) > 30_000


# ---------------------------------------------------------------- refusals write nothing
def test_refusals_write_nothing():
    import torch
    from gaussiansplat_amd import backend as B, renderer as R, synthetic
    from gaussiansplat_amd.density import DensityStats, density_params
    n, deg, W, H = 600, 1, 128, 96
    r = synthetic_renderer(n, deg, seed=50)
    cam = synthetic.scene_camera(W)
    stats = DensityStats(r)
    for t in (stats.grad_sum, stats.count, stats.max_extent):
        t.fill_(3)
    snap = [t.clone() for t in (stats.grad_sum, stats.count, stats.max_extent)]
    p = density_params(scene_extent=4.0)

    # accumulate before a backward: no frame at all, then a frame that is rendered only
    r._begin()
    refused(lambda: r.ctx.density_accumulate(stats.struct()))
    R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
    refused(lambda: r.ctx.density_accumulate(stats.struct()))
    dC = torch.as_tensor(synthetic.make_dC(W, H, 50)).cuda()
    # restructure without a plan, with a wrong n_out, after gs_set_model, with an action of 7, with a destination on the model
    act = np.random.default_rng(50).integers(0, 4, n).astype(np.int32)
    c = D.counts(act)
    no = D.n_out(c)
    t_act, t_noise = dev(act, None), dev(np.random.default_rng(51).standard_normal((n, 2, 3)).astype(f32), None)
    widths = [3, 3, 4, 1, 12]
    dst = [torch.full((no + PAD, w), float(SENTINEL), device="cuda") for w in widths]
    g = lambda ts: B.GsGrads(*[t.data_ptr() for t in ts])
    model_snap = [t.clone() for t in _model(r)]
    go = lambda d=None, k=no, a=t_act: r.ctx.density_restructure(a.data_ptr(), t_noise.data_ptr(), d or g(dst), [], [], k)
    refused(go)                                                                 # no plan yet
    assert r.ctx.density_plan(t_act.data_ptr()) == c
    refused(lambda: go(k=no + 1))
    refused(lambda: go(k=no - 1))
    refused(lambda: go(a=t_act.clone()))                                        # a plan, but for another action array
    alias = list(dst); alias[0] = _model(r)[0]
    refused(lambda: go(d=g(alias)))                                             # dst means on the model's means
    alias = list(dst); alias[1] = dst[0]
    refused(lambda: go(d=g(alias)))                                             # two destinations on each other
    src_set = [torch.zeros((n, w), device="cuda") for w in widths]
    alias = [torch.full((no + PAD, w), float(SENTINEL), device="cuda") for w in widths]; alias[4] = src_set[4]
    refused(lambda: r.ctx.density_restructure(t_act.data_ptr(), t_noise.data_ptr(), g(dst), [g(src_set)], [g(alias)], no))   # a set onto its source
    refused(lambda: r.ctx.density_restructure(t_act.data_ptr(), None, g(dst), [], [], no))                                   # splits without noise
    refused(lambda: r.ctx.density_restructure(t_act.data_ptr(), t_noise.data_ptr(), g(dst), [g(src_set)] * 5, [g(src_set)] * 5, no))   # nsets 5
    r.ctx.set_model_device(n, deg, [t.data_ptr() for t in _model(r)])           # the model "changed": the plan is gone
    refused(go)
    bad = act.copy(); bad[n // 2] = 7
    t_bad = dev(bad, None)
    refused(lambda: r.ctx.density_plan(t_bad.data_ptr()))
    refused(lambda: go(a=t_bad))
    bad[n // 2] = -1
    t_bad.copy_(dev(bad, None))
    refused(lambda: r.ctx.density_plan(t_bad.data_ptr()))
    # a bad struct_size, NaN thresholds
    action = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    for field, val in (("struct_size", 24), ("struct_size", 0), ("grad_threshold", math.nan), ("log_shrink", math.nan)):
        q = density_params(scene_extent=4.0)
        setattr(q, field, val)
        refused(lambda: r.ctx.density_decide(stats.struct(), q, action.data_ptr()))
    # the 2-D renderer
    r2 = R.getRenderer("GAUSSIAN_2D", (W, H, 3), (16, 16), None, n)
    r2._begin()
    for call in (lambda: r2.ctx.density_accumulate(stats.struct()), lambda: r2.ctx.density_decide(stats.struct(), p, action.data_ptr()),
                 lambda: r2.ctx.density_plan(t_act.data_ptr()),
                 lambda: r2.ctx.density_restructure(t_act.data_ptr(), t_noise.data_ptr(), g(dst), [], [], no), lambda: r2.ctx.opacity_reset(-4.0)):
        refused(call, code=B.GS_ERR_UNSUPPORTED)
    torch.cuda.synchronize()
    for a, b in zip(snap, (stats.grad_sum, stats.count, stats.max_extent)):
        assert torch.equal(a, b)
    for a, b in zip(model_snap, _model(r)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(bool((t == float(SENTINEL)).all()) for t in dst) and bool((action == -5).all())
    # nothing was left half done: the valid sequence runs
    R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
    R.backward(r, dC)
    stats.reset(); stats.accumulate()
    assert r.ctx.density_plan(t_act.data_ptr()) == c
    go()
    torch.cuda.synchronize()
    assert int(stats.count.sum()) > 0 and not bool((dst[0][:no] == float(SENTINEL)).any())


# ---------------------------------------------------------------- opacity reset
def test_opacity_reset_is_exact():
    import torch
    from gaussiansplat_amd import synthetic
    from gaussiansplat_amd.density import logit, reset_opacity
    from gaussiansplat_amd.optim import Adam
    n, deg = 1281, 1
    scene = synthetic.make_scene(n, 128, 96, deg, seed=60)
    scene["opacities"][5] = np.nan
    scene["opacities"][6] = np.inf
    scene["opacities"][7] = -np.inf
    scene["opacities"][8] = f32(logit(0.01))
    r = synthetic_renderer(n, deg, 0, scene=scene)
    m, v = torch.ones(n, device="cuda"), torch.full((n,), 2.0, device="cuda")
    r._begin()
    mx = float(f32(logit(0.01)))
    o0 = host([r.splatData.opacities])[0]
    r.ctx.opacity_reset(mx, m.data_ptr(), 0)                                    # one moment array, the other NULL
    want, _, _ = D.opacity_reset(o0, mx)
    assert same_bits(host([r.splatData.opacities])[0], want) and np.isnan(want[5, 0]) and want[6, 0] == f32(mx) and want[7, 0] == -np.inf
    assert not m.any() and not torch.signbit(m).any() and bool((v == 2.0).all())
    r.ctx.opacity_reset(-1e30, 0, 0)                                            # both NULL
    want, _, _ = D.opacity_reset(want, -1e30)
    assert same_bits(host([r.splatData.opacities])[0], want)
    # through the module: the opacities' words of Adam's two flat moment buffers, and nothing else of them
    r = synthetic_renderer(n, deg, 0, scene=scene)
    opt = Adam(r, lr=1e-3)
    opt.exp_avg.fill_(1.0); opt.exp_avg_sq.fill_(2.0)
    reset_opacity(r, opt, 0.01)
    want, _, _ = D.opacity_reset(o0, mx)
    assert same_bits(host([r.splatData.opacities])[0], want)
    lo = opt._offsets[3]
    for buf, val in ((opt.exp_avg, 1.0), (opt.exp_avg_sq, 2.0)):
        assert not buf[lo:lo + n].any() and bool((buf[:lo] == val).all()) and bool((buf[lo + n:] == val).all())


# ---------------------------------------------------------------- end to end
RATES = dict(means=1e-3, scales=4e-3, quaternions=2e-3, opacities=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)


def test_end_to_end_restructured_renderer_equals_a_fresh_one():
    import torch
    from gaussiansplat_amd import renderer as R, train as TR
    from gaussiansplat_amd.density import DensityStats, densify_and_prune, density_params
    from gaussiansplat_amd.optim import Adam
    n, Wi, Hi, deg = 3000, 128, 96, 1
    widths = [3, 3, 4, 1, 12]
    start, cam, gt = perturbed_start(n, Wi, Hi, deg)
    r = R.getRenderer("GAUSSIAN_3D", (Wi, Hi, 3), (16, 16), None, start, deterministic=True, tile_parts=1)
    lf = TR.getLossFunction((Wi, Hi, 3), 11, 3, renderer=r)
    opt = Adam(r, lr=RATES)
    stats = DensityStats(r)
    for _ in range(4):
        R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
        _, dC = lf.value_and_grad(r.imageData, gt, want_loss=False)
        R.resetGrads(r)
        R.backward(r, dC)
        stats.accumulate()
        opt.step()
    model = host(_model(r))
    gs, cnt, ext = stats.grad_sum.cpu().numpy(), stats.count.cpu().numpy(), stats.max_extent.cpu().numpy()
    split_flat = lambda flat: [a.reshape(n, w).copy() for a, w in zip(np.split(flat.cpu().numpy(), np.cumsum([w * n for w in widths])[:-1]), widths)]
    moments = [split_flat(opt.exp_avg), split_flat(opt.exp_avg_sq)]
    # thresholds from the run's own statistics, so that every class is populated: half of the visible gaussians densify, half of
    # those split; the faintest tenth is pruned
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = float(np.median((gs / cnt)[cnt > 0]))
    extent = 4.0
    kw = dict(scene_extent=extent, grad_threshold=thr, percent_dense=float(np.exp(np.median(model[1].max(axis=1)))) / extent,
              min_opacity=float(1.0 / (1.0 + np.exp(-np.quantile(model[3], 0.1)))), max_world_fraction=None, max_extent_px=0)
    p = density_params(**kw)
    want = D.decide(model[1], model[3], gs, cnt, ext, f32(p.grad_threshold), f32(p.log_split_scale), f32(p.log_shrink), f32(p.min_opacity_logit),
                    f32(p.log_max_world_scale), p.max_extent_px)
    c = D.counts(want)
    noise = torch.randn((n, 2, 3), generator=torch.Generator("cuda").manual_seed(7), device="cuda").cpu().numpy()
    new, new_m = D.restructure(model, want, noise, log_shrink=f32(p.log_shrink), sets=moments)
    got = densify_and_prune(r, stats, opt, generator=torch.Generator("cuda").manual_seed(7), **kw)
    no = D.n_out(c)
    print("end to end: %d gaussians -> %d (survivors %d, clones %d, splits %d, pruned %d)" % (n, no, *c))
    assert got == dict(survivors=c[0], clones=c[1], splits=c[2], pruned=c[3], n=no) and min(c) > 100
    assert r.nGaussians == no == r.ctx.num_gaussians and opt.step_count == 4
    for a, b in zip(host(_model(r)), new):
        assert same_bits(a, b)
    split_new = lambda flat: [a.reshape(no, w) for a, w in zip(np.split(flat.cpu().numpy(), np.cumsum([w * no for w in widths])[:-1]), widths)]
    for flat, ref in ((opt.exp_avg, new_m[0]), (opt.exp_avg_sq, new_m[1])):
        for a, b in zip(split_new(flat), ref):
            assert same_bits(a, b)
            assert a[:c[0]].any() and not a[c[0]:].any()                        # survivors carried over, new rows zero
    assert stats.grad_sum.numel() == no and not stats.grad_sum.any() and not stats.count.any() and not stats.max_extent.any()
    assert r.splatGrads.flat.numel() == sum(widths) * no and not r.splatGrads.flat.any()
    # a frame and its backward on the changed renderer against a fresh renderer built from copies of the new arrays
    sd = r.splatData
    fresh = R.GaussianRenderer3D(R.SplatData3D(means=sd.means.clone(), scales=sd.scales.clone(), shs=sd.shs.clone(), quaternions=sd.quaternions.clone(),
                                               opacities=sd.opacities.clone()), (Wi, Hi), deg, deterministic=True, tile_parts=1)
    outs = []
    for rr in (r, fresh):
        R.forward(rr, (R.preprocess(rr, cam), R.compactIdxs(rr))[0])
        lfr = lf if rr is r else TR.getLossFunction((Wi, Hi, 3), 11, 3, renderer=rr)
        _, dC = lfr.value_and_grad(rr.imageData, gt, want_loss=False)
        R.resetGrads(rr)
        R.backward(rr, dC)
        g = rr.splatGrads
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (rr.imageData, rr.transmittance, g.Δmeans, g.Δscales, g.Δquaternions, g.Δopacities, g.Δshs)])
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert outs[0][2].any() and outs[0][6].any()
    stats.accumulate()                                                          # the resized statistics take the new frame
    before = opt.exp_avg.clone()
    opt.step()
    torch.cuda.synchronize()
    assert opt.step_count == 5 and not torch.equal(before, opt.exp_avg) and int(stats.count.sum()) > 0
    assert all(np.isfinite(a).all() for a in host(_model(r)))


def test_densify_and_prune_refuses_a_renderer_that_shares_its_gradients_and_honours_max_gaussians():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    from gaussiansplat_amd.density import DensityStats, densify_and_prune
    n, W, H, deg = 1000, 128, 96, 1
    r = synthetic_renderer(n, deg, seed=70)
    second = R.GaussianRenderer3D(r.splatData, (W, H), deg, share_grads_with=r)
    with pytest.raises(ValueError, match="share_grads_with"):
        densify_and_prune(second, DensityStats(second), scene_extent=4.0)
    stats = DensityStats(r)
    _frame(r, synthetic.scene_camera(W), torch.as_tensor(synthetic.make_dC(W, H, 70)).cuda())
    stats.accumulate()
    opac = host([r.splatData.opacities])[0]
    faint = int((opac < f32(math.log(0.2 / 0.8))).sum())
    # every visible gaussian with a gradient would densify: more than max_gaussians, so only the pruning happens
    got = densify_and_prune(r, stats, scene_extent=4.0, grad_threshold=0.0, min_opacity=0.2, max_world_fraction=None, max_gaussians=n)
    assert got == dict(survivors=n - faint, clones=0, splits=0, pruned=faint, n=n - faint) and 0 < faint < n and r.nGaussians == n - faint


# ---------------------------------------------------------------- training with the schedule
def test_training_with_the_controller_changes_n_and_reduces_the_loss():
    from gaussiansplat_amd import renderer as R, train as TR
    from gaussiansplat_amd.density import DensityController
    from gaussiansplat_amd.optim import Adam
    n, Wi, Hi, deg = 3000, 128, 96, 1
    start, cam, gt = perturbed_start(n, Wi, Hi, deg)
    extent = float(np.linalg.norm(start["means"].max(0) - start["means"].min(0)) / 2)
    sixth = {k: v[:n // 6].copy() for k, v in start.items()}
    finals = {}
    for name in ("plain", "density"):
        r = R.getRenderer("GAUSSIAN_3D", (Wi, Hi, 3), (16, 16), None, sixth)
        lf = TR.getLossFunction((Wi, Hi, 3), 11, 3, renderer=r)
        opt = Adam.for_3dgs(r, extent)
        ctl = DensityController(scene_extent=extent, from_iter=5, until_iter=26, interval=10, opacity_reset_interval=0,
                                grad_threshold=2e-6) if name == "density" else None
        losses = TR.train(r, gt, 0.0, lf, iterations=26, camera=cam, optimizer=opt, density=ctl)
        finals[name] = (losses[0], losses[-1], r.nGaussians)
        print("%s: first / final loss after 26 iterations from %d gaussians %.6f / %.6f, N = %d" % (name, n // 6, *finals[name]))
        if ctl is not None:
            print("densify_and_prune ran at", [(it, c) for it, c in ctl.history])
            assert [it for it, _ in ctl.history] == [10, 20] and r.nGaussians != n // 6, ctl.history
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (name, losses[0], losses[-1])
