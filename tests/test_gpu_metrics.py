"""Evaluation metrics on the GPU (gs_image_metrics, metrics.image_metrics / evaluate, train.Evaluator) against the float64
restatement of tests/metrics_ref.py.

The bars: the mean SSIM within 1e-10 absolute, the map within 2^-24 |S| + 1e-10 (one float32 rounding of a double within 1e-10),
MSE and MAE within 1e-12 relative (the terms are exact differences, the sums of fewer than 2^31 terms are in double).  1e-10 is 30
times the measured distance between two float64 summation orders of the formula (3.5e-12, tests/test_metrics_host.py) and 10^5
times below what a float32 evaluation does on `flat_noise`; a lost window tap moves the mean by more than 6e-4."""
import ctypes as C

import numpy as np
import pytest

import metrics_ref as MR
from common import render, same_bits, small_scene_renderer

pytestmark = pytest.mark.gpu

BIG = (3, 49, 193)


def _check(sums, smap, img, gt, S64, weight=None):
    want = MR.sums_of(img, gt, S64, weight)
    assert np.isfinite(sums).all()
    assert abs(sums[3] - want[3]) <= 1e-12 * want[3]
    assert abs(sums[0] - want[0]) <= 1e-12 * want[0], (sums[0], want[0])
    assert abs(sums[1] - want[1]) <= 1e-12 * want[1], (sums[1], want[1])
    assert abs(sums[2] / sums[3] - want[2] / want[3]) <= 1e-10, (sums[2] / sums[3], want[2] / want[3])
    if smap is not None:
        assert smap.dtype == np.float32 and np.all(np.abs(smap.astype(np.float64) - S64) <= 2.0 ** -24 * np.abs(S64) + 1e-10), \
            float(np.abs(smap.astype(np.float64) - S64).max())


@pytest.fixture(scope="module")
def ctx():
    from gaussiansplat_amd import backend as B
    c = B.Context()
    yield c
    c.close()


@pytest.mark.parametrize("name", MR.FAMILIES)
def test_metrics_family_against_the_float64_restatement(ctx, name):
    worst = [0.0, 0.0, 0.0]                                                    # measured, printed before anything is asserted
    got = []
    for shape in MR.SHAPES:
        c = MR.case(name, shape)
        sums, smap = ctx.image_metrics_host(c.img, c.gt, None, True)
        got.append((shape, c, sums, smap))
        over = np.abs(smap.astype(np.float64) - c.S) - 2.0 ** -24 * np.abs(c.S)
        rel = max(abs(sums[k] - c.sums[k]) / c.sums[k] if c.sums[k] else abs(sums[k]) for k in (0, 1))
        worst = [max(worst[0], abs(sums[2] / sums[3] - c.fin.ssim)), max(worst[1], float(over.max())), max(worst[2], rel)]
    print(name, "worst: mean ssim err %.3g, map err beyond one float32 rounding %.3g, mse / mae rel err %.3g" % tuple(worst))
    for shape, c, sums, smap in got:
        assert sums[3] == float(np.prod(shape))                              # w = 1: the count, exactly
        _check(sums, smap, c.img, c.gt, c.S)
        without_map, none = ctx.image_metrics_host(c.img, c.gt, None, False)
        assert none is None and same_bits(without_map, sums), shape           # the map is an output, not an input of the sums


@pytest.mark.parametrize("name", ["uniform", "flat_noise"])
def test_metrics_weights(ctx, name):
    from gaussiansplat_amd import backend as B
    rng = np.random.default_rng(11)
    for shape in ((3, 17, 65), BIG, (2, 5, 40)):
        c = MR.case(name, shape)
        mask = (rng.random(shape[1:]) < 0.4).astype(np.float32)
        wf = (3.0 * rng.random(shape[1:], dtype=np.float32)).astype(np.float32)
        wf[0, 0] = 0.0
        plain, map_plain = ctx.image_metrics_host(c.img, c.gt, None, True)
        for w in (mask, wf):
            sums, smap = ctx.image_metrics_host(c.img, c.gt, w, True)
            _check(sums, smap, c.img, c.gt, c.S, w)
            assert same_bits(smap, map_plain)                                # the map is that of the whole unweighted images
        ones, map_ones = ctx.image_metrics_host(c.img, c.gt, np.ones(shape[1:], np.float32), True)
        assert same_bits(ones, plain) and same_bits(map_ones, map_plain)
        zeros, _ = ctx.image_metrics_host(c.img, c.gt, np.zeros(shape[1:], np.float32), False)
        assert zeros[3] == 0.0 and np.isnan(B.metrics_finish(zeros)).all()


def test_metrics_identical_images(ctx):
    from gaussiansplat_amd import backend as B
    for name, shape in (("uniform", BIG), ("smooth_near", (3, 17, 65)), ("checker", (1, 16, 64))):
        c = MR.case(name, shape)
        sums, smap = ctx.image_metrics_host(c.gt, c.gt, None, True)
        fin = B.metrics_finish(sums)
        assert sums[0] == 0.0 and sums[1] == 0.0 and fin[B.METRIC_PSNR] == np.inf
        assert abs(fin[B.METRIC_SSIM] - 1.0) <= 1e-12 and np.abs(smap - 1.0).max() <= 2.0 ** -23


def _device_call(ctx, img, gt, weight=None, want_map=True):
    import torch
    x, y = (torch.as_tensor(np.array(a, np.float32)).cuda() for a in (img, gt))
    w = torch.as_tensor(np.array(weight, np.float32)).cuda() if weight is not None else None
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    smap = torch.full(tuple(img.shape), float("nan"), device="cuda") if want_map else None
    Cn, H, W = img.shape
    ctx.image_metrics_device(x.data_ptr(), y.data_ptr(), w.data_ptr() if w is not None else 0, W, H, Cn, smap.data_ptr() if want_map else 0, sums.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return sums.cpu().numpy(), smap.cpu().numpy() if want_map else None


def test_metrics_are_bitwise_reproducible(ctx):
    from gaussiansplat_amd import backend as B, synthetic
    c = MR.case("smooth_near", BIG)
    w = np.random.default_rng(3).random(BIG[1:], dtype=np.float32)
    first = ctx.image_metrics_host(c.img, c.gt, w, True)
    again = ctx.image_metrics_host(c.img, c.gt, w, True)
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
    dev = _device_call(ctx, c.img, c.gt, w)
    assert same_bits(first[0], dev[0]) and same_bits(first[1], dev[1])
    fresh = B.Context()
    other = fresh.image_metrics_host(c.img, c.gt, w, True)
    fresh.close()
    assert same_bits(first[0], other[0]) and same_bits(first[1], other[1])
    r, _, W, H = small_scene_renderer(2000, 1)                                # a context that has rendered frames, under two view slots
    for view in (0, 1, 0):
        render(r, synthetic.scene_camera(W, view))
    used = r.ctx.image_metrics_host(c.img, c.gt, w, True)
    assert same_bits(first[0], used[0]) and same_bits(first[1], used[1])


def test_metrics_scratch_follows_the_image_size():
    """one context at 3 x 49 x 193, then 3 x 1 x 1, then 3 x 49 x 193 again: the partial rows of the larger call are still behind the
    smaller one's, and the first result comes back bit for bit"""
    from gaussiansplat_amd import backend as B
    c = B.Context()
    big, tiny = MR.case("uniform", BIG), MR.case("uniform", (3, 1, 1))
    first = c.image_metrics_host(big.img, big.gt, None, True)
    s_tiny, m_tiny = c.image_metrics_host(tiny.img, tiny.gt, None, True)
    _check(s_tiny, m_tiny, tiny.img, tiny.gt, tiny.S)
    again = c.image_metrics_host(big.img, big.gt, None, True)
    c.close()
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])


def test_metrics_refusals_leave_sums_and_map_untouched(ctx):
    """W, H or C <= 0, C H W >= 2^31, a bad mem, a NULL img, gt or sums, a NULL ctx: GS_ERR_INVALID, and sentinel-filled outputs come back
    as they went in"""
    from gaussiansplat_amd import backend as B
    img = np.full((3, 4, 5), 0.5, np.float32); gt = np.full((3, 4, 5), 0.25, np.float32)
    smap = np.full((3, 4, 5), -7.0, np.float32)
    sums = np.full(4, -7.0, np.float64)
    ip, gp, sp = img.ctypes.data, gt.ctypes.data, sums.ctypes.data
    H_, D_ = B.GS_MEM_HOST, B.GS_MEM_DEVICE
    cases = [(ip, gp, sp, 0, 4, 3, H_), (ip, gp, sp, 5, 0, 3, H_), (ip, gp, sp, 5, 4, 0, H_), (ip, gp, sp, -5, 4, 3, H_), (ip, gp, sp, 5, -4, 3, H_),
             (ip, gp, sp, 5, 4, -3, H_), (ip, gp, sp, 5, 4, 3, 2), (ip, gp, sp, 5, 4, 3, -1), (None, gp, sp, 5, 4, 3, H_), (ip, None, sp, 5, 4, 3, H_),
             (ip, gp, None, 5, 4, 3, H_), (ip, gp, sp, 32768, 32768, 2, H_), (ip, gp, sp, 32768, 32768, 2, D_), (ip, gp, sp, 2 ** 31 - 1, 1, 2, H_)]
    for ip_, gp_, sp_, W, H, Cn, mem in cases:
        rc = ctx.L.gs_image_metrics(ctx.h, C.c_void_p(ip_), C.c_void_p(gp_), None, W, H, Cn, C.c_void_p(smap.ctypes.data), C.c_void_p(sp_), mem)
        assert rc == B.GS_ERR_INVALID, (W, H, Cn, mem, rc)
        assert np.all(smap == -7.0) and np.all(sums == -7.0)
    assert ctx.L.gs_image_metrics(None, C.c_void_p(ip), C.c_void_p(gp), None, 5, 4, 3, None, C.c_void_p(sp), H_) == B.GS_ERR_INVALID
    assert np.all(sums == -7.0)
    got, m = ctx.image_metrics_host(img, gt, None, True)                      # the context still works
    assert np.isfinite(got).all() and got[3] == 60.0 and abs(got[1] / got[3] - 0.25) <= 1e-15 and np.isfinite(m).all()


def test_metrics_between_forward_and_backward_change_no_gradient():
    """forward -> gs_image_metrics -> backward gives the gradients of forward -> backward bit for bit (deterministic mode, one wave per
    tile): the call touches neither the frame nor its stage"""
    import torch
    from gaussiansplat_amd import metrics as M, renderer as R, synthetic
    out = []
    for with_metrics in (False, True):
        r, _, W, H = small_scene_renderer(2000, 1)
        cam = synthetic.scene_camera(W)
        dC = torch.as_tensor(synthetic.make_dC(W, H, 4)).cuda()
        gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(8)).cuda()
        render(r, cam)
        image = r.imageData.clone()
        if with_metrics:
            m = M.image_metrics(r, r.imageData, gt, want_map=True)
            assert np.isfinite([m.mse, m.mae, m.ssim, m.psnr]).all() and m.ssim_map.shape == (3, H, W)
            host = M.image_metrics(r.ctx, r.imageData, gt)                    # ... and through the staged path
            assert (host.mse, host.mae, host.ssim, host.psnr) == (m.mse, m.mae, m.ssim, m.psnr)
        R.backward(r, dC)
        torch.cuda.synchronize()
        assert torch.equal(image, r.imageData)
        out.append(r.splatGrads.flat.clone())
    assert out[0].abs().max() > 0 and torch.equal(out[0], out[1])


def test_evaluate_views_one_by_one_and_leaves_the_renderer_as_found():
    import dataclasses
    import torch
    from gaussiansplat_amd import metrics as M, synthetic
    r, _, W, H = small_scene_renderer(2000, 1)
    cams = [dataclasses.replace(synthetic.scene_camera(W, v), id=10 + v) for v in range(3)]
    g = torch.Generator().manual_seed(21)
    targets = [torch.rand((3, H, W), generator=g) for _ in range(2)] + [torch.rand((4, H, W), generator=g)]
    weights = [None, torch.rand((H, W), generator=g), None]
    train_cam = synthetic.scene_camera(W, 5)
    r.background = (0.25, 0.5, 0.75)
    r.active_sh_degree = 0
    render(r, train_cam)
    res = M.evaluate(r, cams, targets, weights, background=(1.0, 0.0, 0.5))
    assert r.camera is train_cam and r.background == (0.25, 0.5, 0.75) and r.active_sh_degree == 0
    assert len(res.per_view) == 3
    render(r, None)                                                           # None: "the last camera" is the training view again
    again = r.imageData.clone()
    render(r, train_cam)
    assert torch.equal(again, r.imageData)
    # each view rendered alone, over the evaluation background
    r.background = (1.0, 0.0, 0.5)
    for v in range(3):
        render(r, cams[v])
        gt = targets[v].cuda()
        if gt.shape[0] == 4:                                                  # straight alpha over the evaluation background, four fp32 operations
            bg = torch.tensor([1.0, 0.0, 0.5], device="cuda")[:, None, None]
            a = gt[3:4]
            gt = gt[:3] * a + bg * (1.0 - a)
        alone = M.image_metrics(r, r.imageData, gt, weights[v])
        got = res.per_view[v]
        assert (alone.mse, alone.mae, alone.ssim, alone.psnr) == (got.mse, got.mae, got.ssim, got.psnr), v
    for k in ("mse", "mae", "ssim", "psnr"):
        assert getattr(res.mean, k) == float(np.mean([getattr(m, k) for m in res.per_view]))
    with pytest.raises(ValueError):
        M.evaluate(r, cams[:2], targets)


def test_evaluate_runs_under_the_2d_renderer():
    import torch
    from gaussiansplat_amd import metrics as M, renderer as R, synthetic
    W, H = 80, 48
    r = R.getRenderer("GAUSSIAN_2D", (W, H, 3), (16, 16), None, synthetic.make_scene_2d(500, W, H, 3))
    render(r, None)
    own = r.imageData.clone()
    other = torch.rand((3, H, W), generator=torch.Generator().manual_seed(2))
    res = M.evaluate(r, None, [own, other])
    assert res.per_view[0].mse == 0.0 and res.per_view[0].psnr == np.inf and abs(res.per_view[0].ssim - 1.0) <= 1e-12
    ref = MR.finish(MR.restate(own.cpu().numpy(), other.numpy())[0])
    got = res.per_view[1]
    assert abs(got.ssim - ref.ssim) <= 1e-10 and abs(got.mse - ref.mse) <= 1e-12 * ref.mse and abs(got.psnr - ref.psnr) <= 1e-10


def test_training_with_an_evaluator_changes_no_loss():
    """six iterations with an Evaluator(every=2) over two views of their own ids: three history entries, and the losses of the same run
    without an evaluator bit for bit"""
    import dataclasses
    import torch
    from gaussiansplat_amd import synthetic, train as TR
    runs = []
    for with_eval in (False, True):
        r, _, W, H = small_scene_renderer(2000, 1)
        cam = synthetic.scene_camera(W, 0)
        g = torch.Generator().manual_seed(33)
        gt = torch.rand((3, H, W), generator=g).cuda()
        ev = None
        if with_eval:
            cams = [dataclasses.replace(synthetic.scene_camera(W, v), id=20 + v) for v in (1, 2)]
            ev = TR.Evaluator(cams, [torch.rand((3, H, W), generator=g) for _ in cams], every=2)
        lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
        losses = TR.train(r, gt, 0.5, lf, iterations=6, camera=cam, evaluator=ev)
        runs.append((losses, ev))
    (plain, _), (with_ev, ev) = runs
    assert np.array(plain, np.float64).tobytes() == np.array(with_ev, np.float64).tobytes(), (plain, with_ev)
    assert [it for it, _ in ev.history] == [1, 3, 5]
    assert all(np.isfinite([m.mse, m.mae, m.ssim, m.psnr]).all() and m.psnr > 0 for _, m in ev.history)
