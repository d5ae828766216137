"""The evaluation metrics without a GPU: the yardstick itself (tests/metrics_ref.py), the statements of csrc/gs_metrics.h in a host
build (tests/metrics_host.cpp), gs_metrics_finish through ctypes, and the argument checks of train.Evaluator."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR
from common import host_program, run_host


def test_the_two_float64_restatements_agree_per_pixel():
    """grouped conv2d with the 121-tap outer product against the separable NumPy pass, over every family and shape: two summation
    orders of one formula.  1e-10 is the bar the kernel is held to (tests/test_gpu_metrics.py); the worst cell is printed."""
    worst = (0.0, "", ())
    for name in MR.FAMILIES:
        for shape in MR.SHAPES:
            c = MR.case(name, shape)
            e = float(np.abs(MR.ssim_map_separable(c.img, c.gt) - c.S).max())
            worst = max(worst, (e, name, shape))
            assert e <= 1e-10, (name, shape, e)
    print("worst distance between the two float64 orders:", worst)


def test_inputs_are_clipped_to_the_data_range():
    for name in MR.FAMILIES:
        c = MR.case(name, (3, 17, 65))
        assert c.img.dtype == np.float32 and c.img.min() >= 0.0 and c.img.max() <= 1.0 and c.gt.min() >= 0.0 and c.gt.max() <= 1.0


@pytest.mark.parametrize("a,b", [(0.7, 0.6), (0.25, 0.75), (1.0, 0.0)])
def test_constant_images_have_the_closed_form_in_the_interior(a, b):
    """constant images: no variance, so the second factor is C2 / C2 and S = (2ab + C1) / (a^2 + b^2 + C1) wherever the window is whole"""
    img, gt = np.full((2, 30, 40), a, np.float32), np.full((2, 30, 40), b, np.float32)
    a64, b64 = float(np.float32(a)), float(np.float32(b))
    want = (2 * a64 * b64 + MR.C1) / (a64 * a64 + b64 * b64 + MR.C1)
    for S in (MR.ssim_map(img, gt), MR.ssim_map_separable(img, gt)):
        inner = S[:, MR.PAD:-MR.PAD, MR.PAD:-MR.PAD]
        assert inner.size and np.abs(inner - want).max() <= 1e-12, np.abs(inner - want).max()
    border = MR.ssim_map(img, gt)[:, 0, 0]
    assert np.all(np.abs(border - want) > 1e-6) or a == b                # the truncated window sees zeros: not the closed form


@pytest.mark.parametrize("d", [0.5, 0.1, -0.03125, 1.0])
def test_psnr_of_a_constant_difference(d):
    gt = np.full((3, 9, 14), 0.0 if d > 0 else 0.5, np.float32)
    img = (gt + np.float32(d)).astype(np.float32)
    d64 = float(img[0, 0, 0]) - float(gt[0, 0, 0])
    fin = MR.finish(MR.restate(img, gt)[0])
    assert abs(fin.psnr - (-20.0 * math.log10(abs(d64)))) <= 1e-12 * max(1.0, abs(fin.psnr))
    assert abs(fin.mae - abs(d64)) <= 1e-15 and abs(fin.mse - d64 * d64) <= 1e-15


def test_a_lost_tap_moves_the_mean_by_four_orders_more_than_the_bar():
    """drop any one of the 11 taps and renormalise: the mean SSIM of `uniform` at 3 x 17 x 65 moves by more than 1e-6, so the 1e-10
    the kernel is held to cannot hide a lost tap"""
    c = MR.case("uniform", (3, 17, 65))
    moved = []
    for t in range(MR.WIN):
        S = MR.ssim_map(c.img, c.gt, g=MR.window(drop=t))
        moved.append(abs(float(S.mean()) - float(c.S.mean())))
    print("mean SSIM moved by", moved)
    assert min(moved) > 1e-6, moved


def test_float32_is_the_wrong_tool_on_flat_images():
    """why the kernels compute in double: a plain float32 evaluation of the same formula is off by more than 1e-4 per pixel on
    `flat_noise`, six orders above the distance between two float64 summation orders"""
    c = MR.case("flat_noise", (3, 49, 193))
    e32 = float(np.abs(MR.ssim_map(c.img, c.gt, torch.float32).astype(np.float64) - c.S).max())
    assert e32 > 1e-4, e32


# ---------------------------------------------------------------- gs_metrics_finish through ctypes (the library, no GPU)
@pytest.fixture(scope="module")
def backend():
    from gaussiansplat_amd import build
    build.build()
    from gaussiansplat_amd import backend as B
    B.load()
    return B


def test_metrics_finish_ordinary_values(backend):
    B = backend
    sums = np.array([0.5, 2.0, 45.0, 50.0])
    o = B.metrics_finish(sums)
    assert o[B.METRIC_MSE] == 0.5 / 50.0 and o[B.METRIC_MAE] == 2.0 / 50.0 and o[B.METRIC_SSIM] == 45.0 / 50.0
    assert abs(o[B.METRIC_PSNR] - 20.0) <= 1e-13                             # -10 log10(0.01)
    ref = MR.finish(sums)
    assert abs(o[B.METRIC_PSNR] - ref.psnr) <= 1e-13 and o[B.METRIC_MSE] == ref.mse


def test_metrics_finish_zero_error_is_infinite_psnr(backend):
    B = backend
    o = B.metrics_finish([0.0, 0.0, 12.0, 12.0])
    assert o[B.METRIC_MSE] == 0.0 and o[B.METRIC_MAE] == 0.0 and o[B.METRIC_SSIM] == 1.0 and o[B.METRIC_PSNR] == np.inf


@pytest.mark.parametrize("s3", [0.0, -1.0, float("nan")])
def test_metrics_finish_without_weight_is_nan(backend, s3):
    B = backend
    o = B.metrics_finish([1.0, 1.0, 1.0, s3])
    assert np.isnan(o).all()


def test_metrics_finish_refuses_null(backend):
    B = backend
    L = B.load()
    buf = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    assert L.gs_metrics_finish(None, buf) == B.GS_ERR_INVALID and L.gs_metrics_finish(buf, None) == B.GS_ERR_INVALID
    assert list(buf) == [1.0, 1.0, 1.0, 1.0]
    assert L.gs_metrics_finish(buf, buf) == 0


# ---------------------------------------------------------------- csrc/gs_metrics.h in a host build
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program("metrics", tmp_path_factory.mktemp("metrics_host"))


def _run_host(host_exe, img, gt, weight=None):
    Cn, H, W = img.shape
    arrays = [np.asarray(a, np.float32) for a in (img, gt) + ((weight,) if weight is not None else ())]
    sums, fin, S = run_host(host_exe, [], np.array([Cn, H, W, int(weight is not None)], np.int32).tobytes(), arrays,
                            [(np.float64, 4), (np.float64, 4), (np.float64, img.size)])
    return sums, fin, S.reshape(img.shape)


@pytest.mark.parametrize("name,shape", [("uniform", (3, 17, 65)), ("flat_noise", (2, 33, 129)), ("two_consts", (3, 2, 3))],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_header_statements_reproduce_the_restatement(host_exe, name, shape):
    """the text the kernels execute -- window, planes, the 11-tap sum, the pixel formula, finish -- compiled for the host: per pixel
    within 1e-10 of the float64 restatement; the sums as the kernel is held to them"""
    c = MR.case(name, shape)
    w = np.random.default_rng(5).random(shape[1:], dtype=np.float32)
    for weight in (None, w):
        sums, fin, S = _run_host(host_exe, c.img, c.gt, weight)
        want = MR.sums_of(c.img, c.gt, c.S, weight)
        assert np.abs(S - c.S).max() <= 1e-10
        assert abs(sums[0] - want[0]) <= 1e-12 * want[0] and abs(sums[1] - want[1]) <= 1e-12 * want[1]
        assert abs(sums[2] / sums[3] - want[2] / want[3]) <= 1e-10 and abs(sums[3] - want[3]) <= 1e-12 * want[3]
        ref = MR.finish(sums)
        assert fin[0] == ref.mse and fin[1] == ref.mae and fin[2] == ref.ssim and abs(fin[3] - ref.psnr) <= 1e-12 * abs(ref.psnr)


# ---------------------------------------------------------------- train.Evaluator: argument checks (no GPU: nothing is rendered)
def test_evaluator_argument_checks():
    from gaussiansplat_amd import train as TR
    t = [np.zeros((3, 4, 4), np.float32)] * 3
    for bad in (0, -2, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            TR.Evaluator([None] * 3, t, every=bad)
    with pytest.raises(ValueError):
        TR.Evaluator([None] * 2, t, every=1)
    with pytest.raises(ValueError):
        TR.Evaluator([None] * 3, t, every=1, weights=[None] * 4)
    ev = TR.Evaluator(None, t, every=3, weights=[None] * 3, background=(1.0, 1.0, 1.0))
    assert ev.cameras == [None] * 3 and ev.history == [] and ev.every == 3
    assert [it for it in range(9) if ev.due(it)] == [2, 5, 8]
