"""src/loss.jl restatement (oracle/loss_oracle_np.py): known answers + fp64 torch autograd of the gradient."""
import numpy as np
import pytest
import torch

import loss_ref as LR
from oracle import loss_oracle_np as LO


def torch_loss(img, gt, k, lam=0.1, fft=False):
    """fp64 restatement for autograd.  fft=True: the zero-padded 'same' convolution through rfft2 (the window is point
    symmetric, so convolution == correlation) -- the direct grouped conv2d needs ~50 s per 1920x1080x3 backward on a few cores."""
    k4 = torch.as_tensor(k, dtype=torch.float64)[None, None].repeat(img.shape[0], 1, 1, 1)
    conv = lambda t: torch.nn.functional.conv2d(t[None], k4, padding=k.shape[0] // 2, groups=img.shape[0])[0]
    if fft:
        p = k.shape[0] // 2
        Hh, Ww = img.shape[-2] + 2 * p, img.shape[-1] + 2 * p
        kf = torch.fft.rfft2(torch.as_tensor(k, dtype=torch.float64), s=(Hh, Ww))
        conv = lambda t: torch.fft.irfft2(torch.fft.rfft2(t, s=(Hh, Ww)) * kf, s=(Hh, Ww))[..., p:p + img.shape[-2], p:p + img.shape[-1]]
    mux, muy = conv(img), conv(gt)
    s2x, s2y, sxy = conv(img * img) - mux * mux, conv(gt * gt) - muy * muy, conv(img * gt) - mux * muy
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mux * muy + c1) / (mux ** 2 + muy ** 2 + c1) * (2 * sxy + c2) / (s2x + s2y + c2)).mean()
    return (1 - lam) * (img - gt).abs().sum() / (2.0 * img.numel()) + lam * (1 - ssim) / 2.0


def test_kernel_window_known_answers():
    k = LO.kernel_window(11, 1.5)
    assert k.shape == (11, 11) and k.dtype == np.float32
    assert abs(float(k.sum()) - 1.0) < 1e-6
    assert np.allclose(k, k.T) and np.allclose(k, k[::-1, ::-1])           # symmetric: flipkernel is immaterial
    assert k[5, 5] == k.max()                                               # centre ceil(11/2) = 6 (1-based)
    assert np.isclose(k[5, 6] / k[5, 5], np.exp(-1.0), rtol=1e-6)           # exp(-r), not exp(-r^2/2s^2)
    assert np.isclose(k[4, 4] / k[5, 5], np.exp(-np.sqrt(2.0)), rtol=1e-6)
    assert np.allclose(LO.kernel_window(11, 3.0), k, rtol=1e-6)             # sigma cancels in the normalisation


def test_loss_identical_images_and_against_torch():
    rng = np.random.default_rng(0)
    img = rng.random((3, 40, 56), dtype=np.float32)
    gt = rng.random((3, 40, 56), dtype=np.float32)
    k = LO.kernel_window()
    assert abs(LO.loss(img, img, k)) < 1e-6                                 # ssim = 1, L1 = 0
    assert abs(float(LO.ssim_score(img, img, k)) - 1.0) < 1e-6
    want = float(torch_loss(torch.tensor(img, dtype=torch.float64), torch.tensor(gt, dtype=torch.float64), k))
    assert abs(LO.loss(img, gt, k) - want) < 2e-6
    # interior pixel of a constant image: mu = value, variance 0 -> ssim map = 1 there
    c = np.full((1, 32, 32), 0.3, np.float32)
    assert abs(float(LO.ssim_score(c, c, k)) - 1.0) < 1e-6


def test_restatement_of_the_loss_families_equals_torch_loss():
    rng = np.random.default_rng(11)
    img, gt = rng.random((3, 23, 31), dtype=np.float32), rng.random((3, 23, 31), dtype=np.float32)
    for lam in (0.1, 1.0):
        x = torch.tensor(img, dtype=torch.float64, requires_grad=True)
        l = torch_loss(x, torch.tensor(gt, dtype=torch.float64), LO.kernel_window(), lam=lam)
        l.backward()
        loss, grad, smap = LR.restate(img, gt, lam, torch.float64)
        assert abs(loss - float(l.detach())) <= 1e-13 and np.abs(grad - x.grad.numpy()).max() <= 1e-13
        assert smap.shape == img.shape and abs((1 - lam) * np.abs(img - gt).mean(dtype=np.float64) / 2 + lam * (1 - smap.mean()) / 2 - loss) <= 1e-13
    assert LR.restate(img, gt, 0.1, torch.float32)[1].dtype == np.float32


def test_loss_family_inputs_are_what_they_are_named():
    for name in LR.FAMILIES:
        for shape in ((3, 17, 65), (3, 2, 3), (1, 1, 1)):
            img, gt = LR.family(name, *shape, np.random.default_rng(3))
            assert img.shape == gt.shape == shape and img.dtype == gt.dtype == np.float32
            assert img.flags.c_contiguous and gt.flags.c_contiguous
            if name == "two_consts":
                assert not np.any(img == gt)
            elif name != "impulse":                                          # the planted ties: sign(0) = 0
                assert np.array_equal(img[0, :3, :5], gt[0, :3, :5]) and np.array_equal(img[-1, -7:, -9:], gt[-1, -7:, -9:])
    img, gt = LR.family("impulse", 3, 49, 193, np.random.default_rng(3))
    assert not gt.any() and sorted(zip(*np.nonzero(img[1]))) == [(0, 0), (15, 63), (16, 64), (48, 192)]
    img, gt = LR.family("range", 3, 49, 193, np.random.default_rng(3))
    assert img.min() < 0 and img.max() > 1 and np.array_equal(img[0, :3, :5], gt[0, :3, :5]) and np.array_equal(img[2, -7:, -9:], gt[2, -7:, -9:])
    img, gt = LR.family("step", 1, 16, 67, np.random.default_rng(3))
    assert np.array_equal(np.nonzero(img[0, 5] != gt[0, 5])[0], [64])      # the edges at x = 64 and x = 65


@pytest.mark.parametrize("name", LR.FAMILIES)
def test_loss_family_bars_cannot_hide_a_lost_tap(name):
    """The GPU tests allow a kernel FACTOR x the float32 restatement's own error (tests/loss_ref.py).  That allowance itself is
    capped here over the whole matrix: for the sharp families below the window's folded corner weight (four taps of 1.4e-4,
    5.5e-4 in all; with that weight zeroed, or the halo one column short, the kernel was 100 to 10 000 x over its bars on every
    family), for the cancelling ones at 2e-2.  Measured worst: sharp 5.2e-6 (checker,
    lam = 1, 3x1x1), cancelling 2.2e-3 (two_consts, lam = 1)."""
    cap = LR.CAP_SHARP if name in LR.SHARP else LR.CAP_CANCELLING
    assert all(LR.FACTOR < f <= 16.0 for f in LR.RAISED.values()) and LR.FACTOR == 4.0
    for lam in LR.LAMS:
        for shape in LR.SHAPES:
            img, gt, b = LR.case(name, shape, lam)
            assert np.abs(b.grad).max() > 0.0 and np.isfinite(b.grad).all(), (name, lam, shape)
            assert LR.FACTOR * b.e_max <= cap and LR.FACTOR * b.e_l2 <= cap, (name, lam, shape, b.e_max, b.e_l2)
            assert LR.factor(name, shape, "max") * max(b.e_max, b.e_l2) <= cap                  # a raised factor stays under it too
            assert b.e_loss > 0.0 and np.isfinite(b.loss)


def test_fft_form_of_the_torch_reference_equals_the_direct_one():
    rng = np.random.default_rng(5)
    img = rng.random((3, 37, 50)); gt = rng.random((3, 37, 50))
    k = LO.kernel_window()
    g = []
    for fft in (False, True):
        x = torch.tensor(img, dtype=torch.float64, requires_grad=True)
        l = torch_loss(x, torch.tensor(gt, dtype=torch.float64), k, fft=fft)
        l.backward()
        g.append((float(l), x.grad.numpy().copy()))
    assert abs(g[0][0] - g[1][0]) < 1e-13 and np.abs(g[0][1] - g[1][1]).max() < 1e-13
