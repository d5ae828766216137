"""MCMC densification on the device (gs_mcmc_plan / _sample / _relocate / _noise / _regularize, gaussiansplat_amd.mcmc) against the NumPy
restatement of include/gsplat.h (tests/mcmc_ref.py): CDF, dead list, draws, noise and regulariser gradients bit for bit; the relocation's
opacity and scales within one float32 ulp (both sides evaluate in double and round once, tests/test_mcmc_host.py), everything it copies and
everything it must not touch bit for bit; the refusals; growth through mcmc.grow; a short training run with the MCMC schedule."""
import functools
import math

import numpy as np
import pytest

import mcmc_ref as M
from common import dev, host, refused, same_bits, synthetic_renderer

pytestmark = pytest.mark.gpu

f32 = np.float32
MIN_OPACITY = 0.005
MIN_LOGIT = math.log(MIN_OPACITY / (1.0 - MIN_OPACITY))
SENTINEL = -7


_renderer = functools.partial(synthetic_renderer, W=64, H=64)


def _model(r):
    sd = r.splatData
    return [sd.means, sd.scales, sd.quaternions, sd.opacities, sd.shs]


def _within_one_ulp(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, f32)
    return bool(np.all(np.abs(a - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)))


def _set_opacities(r, o):
    r.splatData.opacities.copy_(dev(np.asarray(o, f32).reshape(-1, 1)))


def _plan(r, n):
    """(cdf uint64 [n], dead int32 [n] behind a sentinel fill, counts) of a gs_mcmc_plan with the tensors kept for later calls"""
    import torch
    cdf = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    dead = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    r._begin()
    counts = r.ctx.mcmc_plan(MIN_LOGIT, cdf.data_ptr(), dead.data_ptr())
    return cdf, dead, counts


def _opacity_cases(n, seed):
    rng = np.random.default_rng(seed)
    mixed = rng.uniform(-9.0, 9.0, n).astype(f32)
    odd = mixed.copy()
    odd[rng.integers(0, n, max(1, n // 7))] = np.nan
    odd[rng.integers(0, n, max(1, n // 9))] = np.inf
    odd[rng.integers(0, n, max(1, n // 9))] = -np.inf
    odd[rng.integers(0, n, max(1, n // 9))] = f32(MIN_LOGIT)                # exactly at the threshold: not alive
    odd[rng.integers(0, n, max(1, n // 9))] = 30.0                          # a sigmoid that rounds to 1
    return dict(mixed=mixed, all_dead=rng.uniform(-12.0, -5.5, n).astype(f32), none_dead=rng.uniform(-5.0, 20.0, n).astype(f32), odd=odd)


# ---------------------------------------------------------------- plan
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, 70001, 262145])   # 262145: 1025 chunks, two words per scan thread, half of the spans empty
def test_plan_matches_the_reference_bit_for_bit(n):
    r = _renderer(n, 0, seed=n)
    for name, o in _opacity_cases(n, n).items():
        _set_opacities(r, o)
        cdf, dead, counts = _plan(r, n)
        rc, rd, rcounts = M.plan(o, f32(MIN_LOGIT))
        assert counts == rcounts, (name, counts, rcounts)
        assert np.array_equal(cdf.cpu().numpy().view(np.uint64), rc), name
        d = dead.cpu().numpy()
        assert np.array_equal(d[:len(rd)], rd) and (d[len(rd):] == SENTINEL).all(), name   # ascending; the words past the dead count unwritten
        if name == "all_dead":
            assert counts == (0, n, 0)
        if name == "none_dead":
            assert counts[:2] == (n, 0)


# ---------------------------------------------------------------- sample
@pytest.mark.parametrize("n", [4097, 70001])
def test_sample_equals_searchsorted(n):
    import torch
    r = _renderer(n, 0, seed=n + 1)
    o = _opacity_cases(n, n + 1)["odd"]
    _set_opacities(r, o)
    cdf, _, counts = _plan(r, n)
    rc = M.plan(o, f32(MIN_LOGIT))[0]
    rng = np.random.default_rng(n)
    edge = np.array([0.0, np.nextafter(f32(1), f32(0)), 1.0, -1.0, np.nan, -0.0, np.inf, 0.5], f32)
    for m in (0, 1, 64, 65, 5000):
        u = rng.random(m).astype(f32)
        u[:min(m, len(edge))] = edge[:m]
        tu = dev(u, None) if m else torch.empty(0, device="cuda")
        src = torch.full((m + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        r.ctx.mcmc_sample(cdf.data_ptr(), n, tu.data_ptr(), m, src.data_ptr())
        s = src.cpu().numpy()
        assert (s[m:] == SENTINEL).all()
        if m:
            assert np.array_equal(s[:m], M.sample(rc, u)), m
    # total == 0: nothing is written (decided on the device: no synchronise)
    _set_opacities(r, np.full(n, -9.0, f32))
    cdf0, _, counts0 = _plan(r, n)
    assert counts0 == (0, n, 0)
    src = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
    r.ctx.mcmc_sample(cdf0.data_ptr(), n, dev(rng.random(64).astype(f32)).data_ptr(), 64, src.data_ptr())
    assert bool((src == SENTINEL).all())


# ---------------------------------------------------------------- relocate
def _moment_sets(model, seed):
    """two gradient-shaped sets of random floats: a full one, and one with NULL arrays"""
    import torch
    from gaussiansplat_amd import backend as B
    g = torch.Generator(device="cuda").manual_seed(seed)
    full = [torch.randn(t.shape, generator=g, device="cuda") for t in model]
    part = [None, torch.randn(model[1].shape, generator=g, device="cuda"), None, torch.randn(model[3].shape, generator=g, device="cuda"), None]
    structs = [B.GsGrads(*[t.data_ptr() if t is not None else None for t in s]) for s in (full, part)]
    return [full, part], structs


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("from_plan", [True, False])
def test_relocate_matches_the_reference(deg, from_plan):
    n = 4097
    r = _renderer(n, deg, seed=40 + deg)
    rng = np.random.default_rng(41 + deg)
    o = rng.uniform(-4.0, 6.0, n).astype(f32)
    sources = np.array([7, 300, 1024, 2049, 4000, 4096])
    o[sources] = np.array([-1.0, -4.5, 0.0, 2.0, 5.0, 12.0], f32)           # from barely alive (drawn twice: its copies clamp at min_opacity) to nearly opaque
    dead_rows = np.setdiff1d(rng.choice(n, 420, replace=False), sources)[:400]
    o[dead_rows] = -8.0
    _set_opacities(r, o)
    src = np.repeat(sources, [1, 2, 49, 50, 51, 200]).astype(np.int32)
    rng.shuffle(src)
    src = np.concatenate([src, np.array([-1, n, 2 ** 31 - 1], np.int32)])    # out of range: no-ops, not counted
    if not from_plan:
        src = np.concatenate([src, sources[2:4].astype(np.int32)])          # two draws whose DESTINATION is out of range: no-ops too
    m = len(src)
    cdf, dead, counts = _plan(r, n)
    assert counts[1] == 400 and m == (356 if from_plan else 358)
    if from_plan:
        dst = np.sort(dead_rows)[:m].astype(np.int32)
        dst_ptr = None
    else:
        free = np.setdiff1d(np.arange(n), sources)
        dst = rng.choice(free, m, replace=False).astype(np.int32)           # alive or dead, pairwise distinct, no source
        dst[-2] = -3; dst[-1] = n
        t_dst = dev(dst, None)
        dst_ptr = t_dst.data_ptr()
    sets, structs = _moment_sets(_model(r), 42)
    before = host(_model(r))
    sets_before = [[None if t is None else host([t])[0] for t in s] for s in sets]
    t_src = dev(src, None)
    r.ctx.mcmc_relocate(t_src.data_ptr(), dst_ptr, m, MIN_OPACITY, structs)
    after = host(_model(r))
    new, new_sets, cnt = M.relocate(before, src, dst, MIN_OPACITY, sets_before)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    assert sorted(cnt[sources].tolist()) == [1, 2, 49, 50, 51, 200] and cnt.sum() == ok.sum()
    touched = np.zeros(n, bool)
    touched[sources] = True; touched[dst[ok]] = True
    for i in (0, 2, 4):                                                      # means, quaternions, SH rows: copied, or kept, bit for bit
        assert same_bits(after[i], new[i]), i
    for i in (1, 3):                                                         # scales, opacities: the statement's values within one ulp; the rest every bit
        assert same_bits(after[i][~touched], before[i][~touched]), i
        assert _within_one_ulp(after[i][touched], new[i][touched]), i
        assert same_bits(after[i][dst[ok]], after[i][src[ok]]), i            # a destination carries exactly its source's new values
    assert (after[3][sources] < before[3][sources]).all() and (after[1][sources] < before[1][sources]).all()
    for s_after, s_before in zip([[None if t is None else host([t])[0] for t in s] for s in sets], sets_before):
        for a, b in zip(s_after, s_before):
            if b is None:
                continue
            assert same_bits(a[~touched], b[~touched])
            assert not a[touched].view(np.uint32).any()                      # +0, every bit
    # a fresh plan: what was dead and relocated is alive now (its source's corrected opacity is above the threshold or clamped at it)
    if from_plan:
        _, _, c2 = _plan(r, n)
        clamped = int((after[3][np.sort(dead_rows)[:m][ok], 0] <= f32(MIN_LOGIT)).sum())
        assert c2[1] == 400 - int(ok.sum()) + clamped + int((after[3][sources, 0] <= f32(MIN_LOGIT)).sum())


# ---------------------------------------------------------------- growth
def test_grow_extends_the_model_and_the_renderer_renders():
    import torch
    from gaussiansplat_amd import mcmc, renderer as R, synthetic
    from gaussiansplat_amd.optim import Adam
    n, deg, W = 4097, 1, 64
    r = _renderer(n, deg, seed=50)
    opt = Adam(r, lr=1e-3)
    opt.exp_avg.normal_(); opt.exp_avg_sq.uniform_()
    opt.step_count = 5
    gen = torch.Generator(device="cuda").manual_seed(50)
    with pytest.raises(ValueError, match="share_grads_with"):
        mcmc.grow(R.GaussianRenderer3D(r.splatData, (W, W), deg, share_grads_with=r), cap_max=10 ** 6)
    with pytest.raises(ValueError, match="another renderer"):
        mcmc.grow(_renderer(10, deg, seed=51), opt, cap_max=10 ** 6)
    for cap, want in ((5000, int(1.05 * n)), (4400, 4400), (4400, 4400)):
        n0 = r.nGaussians
        before = host(_model(r))
        mom_before = [m.clone() for m in (opt.exp_avg, opt.exp_avg_sq)]
        off_before = opt._offsets
        got = mcmc.grow(r, opt, cap_max=cap, generator=gen)
        assert got["n"] == want == r.nGaussians == min(cap, int(1.05 * n0)) and got["added"] == want - n0
        after = host(_model(r))
        assert all(a.shape[0] == want for a in after) and opt.step_count == 5 and opt.exp_avg.numel() == r.splatGrads.flat.numel()
        if not got["added"]:
            assert got["src"] is None and all(same_bits(a, b) for a, b in zip(after, before))
            continue
        src = got["src"].cpu().numpy()
        ext = [np.concatenate([b, np.zeros((want - n0, b.shape[1]), f32)]) for b in before]
        new, _, cnt = M.relocate(ext, src, np.arange(n0, want), MIN_OPACITY)
        for i in (0, 2, 4):                                                  # the old rows unchanged, the new ones copies of their sources
            assert same_bits(after[i], new[i])
        srcs = cnt > 0
        for i in (1, 3):
            assert same_bits(after[i][:n0][~srcs[:n0]], before[i][~srcs[:n0]]) and _within_one_ulp(after[i], new[i])
        # moments: old rows carried over, rows of sources and of the new gaussians +0
        for mb, ma in zip(mom_before, (opt.exp_avg, opt.exp_avg_sq)):
            for ob, oa, wd in zip(off_before, opt._offsets, (3, 3, 4, 1, after[4].shape[1])):
                b = mb[ob:ob + n0 * wd].reshape(n0, wd).cpu().numpy()
                a = ma[oa:oa + want * wd].reshape(want, wd).cpu().numpy()
                assert same_bits(a[:n0][~srcs[:n0]], b[~srcs[:n0]]) and not a[:n0][srcs[:n0]].any() and not a[n0:].any()
    cam = synthetic.scene_camera(W)
    R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
    img = r.imageData.cpu().numpy()
    assert np.isfinite(img).all() and img.max() > 0


# ---------------------------------------------------------------- noise, regularisers
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_noise_matches_the_reference_bit_for_bit(n):
    r = _renderer(n, 0, seed=60 + n)
    rng = np.random.default_rng(60 + n)
    q = (rng.normal(0, 1, (n, 4)) * rng.uniform(0.2, 3.0, (n, 1))).astype(f32)      # raw: not normalised
    r.splatData.quaternions.copy_(dev(q, None))
    o = rng.uniform(-9.0, 3.0, n).astype(f32)
    o[:min(n, 3)] = np.array([MIN_LOGIT, -5.0, -5.6], f32)[:min(n, 3)]           # sig on both sides of gate_t
    _set_opacities(r, o)
    z = rng.normal(0, 1, (n, 3)).astype(f32)
    if n > 40:
        z[10:20] = 0.0
        z[21] = np.inf                                                        # the result would not be finite: the mean is kept
    tz = dev(z, None)
    r._begin()
    for lr in (80.0, 1e-3):
        before = host(_model(r))
        r.ctx.mcmc_noise(tz.data_ptr(), lr, 100.0, 0.005)
        after = host(_model(r))
        ref = M.noise(before[0], before[1], before[2], before[3], z, lr, 100.0, 0.005)
        assert same_bits(after[0], ref)
        assert all(same_bits(a, b) for a, b in zip(after[1:], before[1:]))
        if n > 40:
            assert same_bits(after[0][10:20], before[0][10:20]) and same_bits(after[0][21], before[0][21]) and (after[0] != before[0]).any()
    before = host(_model(r))
    r.ctx.mcmc_noise(tz.data_ptr(), 0.0)                                     # lr == 0: nothing
    assert all(same_bits(a, b) for a, b in zip(host(_model(r)), before))


def test_regularize_matches_the_reference_bit_for_bit():
    import torch
    from gaussiansplat_amd import backend as B, mcmc
    n = 4097
    r = _renderer(n, 1, seed=70)
    rng = np.random.default_rng(70)
    _set_opacities(r, rng.uniform(-9.0, 20.0, n).astype(f32))
    model = host(_model(r))
    d_op = dev(rng.normal(0, 1e-4, (n, 1)).astype(f32))
    d_sc = dev(rng.normal(0, 1e-4, (n, 3)).astype(f32))
    c_o, c_s = M.reg_coefficients(0.01, 0.02, n)
    r._begin()
    h_op, h_sc = host([d_op, d_sc])
    r.ctx.mcmc_regularize(B.GsGrads(None, d_sc.data_ptr(), None, d_op.data_ptr(), None), float(c_o), float(c_s))
    ref_o, ref_s = M.regularize(h_op, h_sc, model[3], model[1], c_o, c_s)
    a_op, a_sc = host([d_op, d_sc])
    assert same_bits(a_op.reshape(-1), ref_o) and same_bits(a_sc, ref_s) and (a_op != h_op).any() and (a_sc != h_sc).any()
    # a NULL d_scales, then a zero coefficient: that half is skipped
    r.ctx.mcmc_regularize(B.GsGrads(None, None, None, d_op.data_ptr(), None), float(c_o), float(c_s))
    ref_o2, _ = M.regularize(a_op, None, model[3], model[1], c_o, c_s)
    b_op, b_sc = host([d_op, d_sc])
    assert same_bits(b_op.reshape(-1), ref_o2) and same_bits(b_sc, a_sc)
    r.ctx.mcmc_regularize(B.GsGrads(None, d_sc.data_ptr(), None, d_op.data_ptr(), None), 0.0, float(c_s))
    c_op, c_sc = host([d_op, d_sc])
    assert same_bits(c_op, b_op) and same_bits(c_sc, M.regularize(None, b_sc, model[3], model[1], c_o, c_s)[1])
    assert all(same_bits(a, b) for a, b in zip(host(_model(r)), model))
    # through the module: the renderer's own gradient buffer, coefficients lambda / N and lambda / (3 N)
    r.splatGrads.flat.zero_()
    mcmc.regularize(r, opacity_reg=0.01, scale_reg=0.02)
    g_op, g_sc = host([r.splatGrads.Δopacities.reshape(n, 1), r.splatGrads.Δscales.reshape(n, 3)])
    z_o, z_s = M.regularize(np.zeros(n, f32), np.zeros((n, 3), f32), model[3], model[1], c_o, c_s)
    assert same_bits(g_op.reshape(-1), z_o) and same_bits(g_sc, z_s)
    assert not bool(r.splatGrads.Δmeans.any()) and not bool(r.splatGrads.Δshs.any())


# ---------------------------------------------------------------- refusals leave the model untouched
def test_refusals_write_nothing():
    import torch
    from gaussiansplat_amd import backend as B, renderer as R, synthetic
    n, deg, W = 600, 1, 64
    r = _renderer(n, deg, seed=80)
    o = np.random.default_rng(80).uniform(-4.0, 6.0, n).astype(f32)
    o[:50] = -8.0
    _set_opacities(r, o)
    snap = [t.clone() for t in _model(r)]
    src = dev(np.full(20, 100, np.int32), None)
    dst = dev(np.arange(200, 220, dtype=np.int32), None)
    z = torch.randn((n, 3), device="cuda")
    grad_arrays = [torch.zeros_like(t) for t in _model(r)]
    grads = B.GsGrads(*[t.data_ptr() for t in grad_arrays])
    sets, structs = _moment_sets(_model(r), 81)
    sets_snap = [[None if t is None else t.clone() for t in s] for s in sets]

    r._begin()
    rel = lambda s=src.data_ptr(), d=dst.data_ptr(), m=20, mo=MIN_OPACITY, st=structs: r.ctx.mcmc_relocate(s, d, m, mo, st)
    refused(lambda: rel(m=-1))
    for mo in (0.0, 1.0, -0.5, 1.5, math.nan):
        refused(lambda: rel(mo=mo))
    refused(lambda: rel(st=structs * 3))                                     # nsets 6
    refused(lambda: rel(s=None))                                             # NULL src with m > 0
    refused(lambda: rel(d=None))                                             # no plan yet
    cdf, dead, counts = _plan(r, n)
    assert counts[1] == 50
    refused(lambda: rel(d=None, m=51))                                       # more than the plan's dead count
    r.ctx.set_model_device(n, deg, [t.data_ptr() for t in _model(r)])        # the model "changed": the plan is gone
    refused(lambda: rel(d=None))
    for args in ((math.nan, 100.0, 0.005), (1.0, math.inf, 0.005), (1.0, 100.0, math.nan), (-1.0, 100.0, 0.005), (math.inf, 100.0, 0.005)):
        refused(lambda: r.ctx.mcmc_noise(z.data_ptr(), *args))
    refused(lambda: r.ctx.mcmc_noise(r.splatData.means.data_ptr(), 1.0))     # z on the model's means
    refused(lambda: r.ctx.mcmc_noise(r.splatData.shs.data_ptr() + 4, 1.0))   # ... inside its SH rows
    refused(lambda: r.ctx.mcmc_noise(None, 1.0))
    refused(lambda: r.ctx.mcmc_plan(math.nan, cdf.data_ptr(), dead.data_ptr()))
    refused(lambda: r.ctx.mcmc_sample(cdf.data_ptr(), -1, z.data_ptr(), 4, src.data_ptr()))
    refused(lambda: r.ctx.mcmc_regularize(grads, math.nan, 0.0))
    r2 = R.getRenderer("GAUSSIAN_2D", (W, W, 3), (16, 16), None, n)
    r2._begin()
    for call in (lambda: r2.ctx.mcmc_plan(MIN_LOGIT, cdf.data_ptr(), dead.data_ptr()),
                 lambda: r2.ctx.mcmc_sample(cdf.data_ptr(), n, z.data_ptr(), 4, src.data_ptr()),
                 lambda: r2.ctx.mcmc_relocate(src.data_ptr(), dst.data_ptr(), 20, MIN_OPACITY, []),
                 lambda: r2.ctx.mcmc_noise(z.data_ptr(), 1.0), lambda: r2.ctx.mcmc_regularize(grads, 0.1, 0.1)):
        refused(call, code=B.GS_ERR_UNSUPPORTED)
    torch.cuda.synchronize()
    for a, b in zip(snap, _model(r)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for sa, sb in zip(sets_snap, sets):
        for a, b in zip(sa, sb):
            assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32))
    # nothing was left half done: the valid sequence runs, m == 0 changes nothing, and the regulariser leaves the frame standing
    cam = synthetic.scene_camera(W)
    R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
    R.backward(r, torch.as_tensor(synthetic.make_dC(W, W, 80)).cuda())
    r.ctx.mcmc_regularize(r._grads, 1e-5, 1e-5)
    R.backward(r, torch.as_tensor(synthetic.make_dC(W, W, 80)).cuda())       # the frame stands: a second backward is legal without a forward
    keep = _plan(r, n)                                                       # (the dead list is the caller's: it has to live until the relocation)
    assert keep[2][1] == 50
    rel(d=None, m=0)
    for a, b in zip(snap, _model(r)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rel(d=None)
    torch.cuda.synchronize()
    assert not torch.equal(snap[3], _model(r)[3])
    refused(lambda: rel(d=None))                                             # the relocation dropped its own plan
    refused(lambda: R.backward(r, torch.as_tensor(synthetic.make_dC(W, W, 80)).cuda()))   # ... and the frame, like an optimiser step


# ---------------------------------------------------------------- training with the schedule
def test_training_with_the_mcmc_controller():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.mcmc import MCMCController
    from gaussiansplat_amd.optim import Adam
    n, W, deg, cap = 2000, 64, 1, 2400
    target = synthetic.make_scene(n, W, W, deg, seed=1)
    cam = synthetic.scene_camera(W)
    rt = R.getRenderer("GAUSSIAN_3D", (W, W, 3), (16, 16), None, target)
    R.forward(rt, (R.preprocess(rt, cam), R.compactIdxs(rt))[0])
    gt = rt.imageData.clone()
    start = {k: v.copy() for k, v in target.items()}
    start["shs"] = (start["shs"] + 0.2 * np.random.default_rng(2).standard_normal(start["shs"].shape)).astype(f32)
    start["opacities"][np.random.default_rng(3).choice(n, 150, replace=False)] = -8.0        # dead from the start
    want, k = [], n
    for _ in range(4):                                                       # the closed form: 5 % per interval up to the cap
        k = min(cap, int(1.05 * k)); want.append(k)
    runs = []
    for _ in range(2):
        r = R.getRenderer("GAUSSIAN_3D", (W, W, 3), (16, 16), None, {k_: v.copy() for k_, v in start.items()}, deterministic=True, tile_parts=1)
        lf = TR.getLossFunction((W, W, 3), 11, 3, renderer=r)
        opt = Adam.for_3dgs(r, 4.0)
        ctl = MCMCController(cap_max=cap, from_iter=10, interval=10, generator=torch.Generator(device="cuda").manual_seed(7))
        losses, sizes, dead_after = [], [], []
        for it in range(1, 41):
            losses.append(float(TR.trainStep(r, gt, 0.0, lf, cam, optimizer=opt, density=ctl)))
            sizes.append(r.nGaussians)
            assert r.nGaussians <= cap
            if it % 10 == 0:
                assert ctl.history[-1][0] == it
                if ctl.history[-1][1]["alive"] > 0:
                    dead_after.append(_plan(r, r.nGaussians)[2][1])
        hist = ctl.history
        print("MCMC run: N", [h[1]["n"] for h in hist], "dead / relocated", [(h[1]["dead"], h[1]["relocated"]) for h in hist], "dead afterwards", dead_after,
              "loss %.5f -> %.5f" % (losses[0], losses[-1]))
        assert [h[0] for h in hist] == [10, 20, 30, 40] and [h[1]["n"] for h in hist] == want == [sizes[9], sizes[19], sizes[29], sizes[39]]
        assert hist[0][1]["dead"] >= 150 and hist[0][1]["relocated"] == hist[0][1]["dead"]
        assert dead_after == [0, 0, 0, 0]
        assert np.isfinite(losses).all() and opt.exp_avg.numel() == r.splatGrads.flat.numel()
        runs.append((sizes, [None if h[1][key] is None else h[1][key].cpu().numpy() for h in hist for key in ("relocate_src", "grow_src")]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):                                 # equal seeds: bit-equal draws
        assert (a is None and b is None) or np.array_equal(a, b)
    # SGD has no optimiser to take the rate from: means_lr, or a ValueError
    with pytest.raises(ValueError):
        TR.trainStep(r, gt, 1e-3, lf, cam, density=MCMCController(cap_max=cap))
