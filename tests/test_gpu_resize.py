"""One renderer and one optim.Adam through both strategies that change the number of gaussians, in turn: density.densify_and_prune, mcmc.grow,
densify_and_prune again, with a frame, a backward and a step between them.  After every resize the renderer, the ctx, the gradient buffer,
the optimiser and the statistics agree on the new size; at the end a frame and its backward equal, bit for bit, those of a fresh renderer
built from clones of the arrays (the comparison of test_gpu_density.py::test_end_to_end_restructured_renderer_equals_a_fresh_one)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES = dict(means=1e-3, scales=4e-3, quaternions=2e-3, opacities=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)


def _views(g):
    return g.Δmeans, g.Δscales, g.Δquaternions, g.Δopacities, g.Δshs


def _agree(r, opt, stats, steps):
    n = r.nGaussians
    assert n == r.ctx.num_gaussians == r.splatData.means.shape[0]
    g = r._splatGrads
    s = r._grads
    assert [int(p) for p in (s.d_means, s.d_scales, s.d_quats, s.d_opacities, s.d_shs)] == [v.data_ptr() for v in _views(g)]
    assert [tuple(v.shape) for v in _views(g)] == [(n, 3), (n, 3), (n, 4), (n, 1), (n, r.splatData.shs.shape[1])]
    assert opt._numel == g.flat.numel() == opt.exp_avg.numel() == opt.exp_avg_sq.numel()
    assert opt.step_count == steps                                              # a resize is no step
    assert stats.grad_sum.numel() == stats.count.numel() == stats.max_extent.numel() == n
    assert not stats.grad_sum.any() and not stats.count.any() and not stats.max_extent.any()


def test_one_renderer_one_adam_through_densify_grow_densify():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.density import DensityStats, densify_and_prune
    from gaussiansplat_amd.mcmc import grow
    from gaussiansplat_amd.optim import Adam
    n, Wi, Hi, deg = 300, 64, 48, 1
    target = synthetic.make_scene(n, Wi, Hi, deg, seed=1)
    cam = synthetic.scene_camera(Wi)
    rt = R.getRenderer("GAUSSIAN_3D", (Wi, Hi, 3), (16, 16), None, target)
    R.forward(rt, (R.preprocess(rt, cam), R.compactIdxs(rt))[0])
    gt = rt.imageData.clone()
    start = {k: v.copy() for k, v in target.items()}
    start["shs"] = (start["shs"] + 0.2 * np.random.default_rng(2).standard_normal(start["shs"].shape)).astype(np.float32)
    start["opacities"] = (start["opacities"] - 0.5).astype(np.float32)
    r = R.getRenderer("GAUSSIAN_3D", (Wi, Hi, 3), (16, 16), None, start, deterministic=True, tile_parts=1)
    lf = TR.getLossFunction((Wi, Hi, 3), 11, 3, renderer=r)
    opt = Adam(r, lr=RATES)
    stats = DensityStats(r)
    gen = torch.Generator("cuda").manual_seed(7)

    def iteration():
        R.forward(r, (R.preprocess(r, cam), R.compactIdxs(r))[0])
        _, dC = lf.value_and_grad(r.imageData, gt, want_loss=False)
        R.resetGrads(r)
        R.backward(r, dC)
        stats.accumulate()
        opt.step()

    def densify():
        """thresholds from the run's own statistics, so that every class is populated: half of the visible gaussians densify, half of those
        split; the faintest tenth is pruned"""
        torch.cuda.synchronize()
        gs, cnt = stats.grad_sum.cpu().numpy(), stats.count.cpu().numpy()
        scales, opac = r.splatData.scales.cpu().numpy(), r.splatData.opacities.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            thr = float(np.median((gs / cnt)[cnt > 0]))
        extent = 4.0
        before = r.nGaussians
        got = densify_and_prune(r, stats, opt, generator=gen, scene_extent=extent, grad_threshold=thr,
                                percent_dense=float(np.exp(np.median(scales.max(axis=1)))) / extent,
                                min_opacity=float(1.0 / (1.0 + np.exp(-np.quantile(opac, 0.1)))), max_world_fraction=None, max_extent_px=0)
        print("densify_and_prune: %d -> %s" % (before, got))
        assert min(got["survivors"], got["clones"], got["splits"], got["pruned"]) > 0, got       # an empty class fails the test
        assert got["n"] == got["survivors"] + got["clones"] + 2 * got["splits"] == r.nGaussians != before
        return got

    steps = 0
    for _ in range(3):
        iteration(); steps += 1
    densify()
    _agree(r, opt, stats, steps)
    iteration(); steps += 1
    before = r.nGaussians
    got = grow(r, opt, cap_max=10 * n, growth=1.25, generator=gen)
    print("grow: %d -> %d" % (before, got["n"]))
    assert got["added"] == int(1.25 * before) - before > 0 and got["n"] == r.nGaussians == before + got["added"]
    stats.resize(r.nGaussians)                                                  # grow knows no statistics: their owner follows
    _agree(r, opt, stats, steps)
    for _ in range(2):
        iteration(); steps += 1
    densify()
    _agree(r, opt, stats, steps)
    assert not r.splatGrads.flat.any()
    # a frame and its backward on the renderer that was resized three times against a fresh renderer built from copies of its arrays
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
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (rr.imageData, rr.transmittance) + _views(rr.splatGrads)])
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert outs[0][2].any() and outs[0][6].any()
    stats.accumulate()                                                          # and the run goes on: statistics and a step at the new size
    before = opt.exp_avg.clone()
    opt.step()
    torch.cuda.synchronize()
    assert opt.step_count == steps + 1 and not torch.equal(before, opt.exp_avg) and int(stats.count.sum()) > 0
