"""The per-view exposure stage without a GPU: the statements of csrc/gs_exposure.h in a host build (tests/exposure_host.cpp) against the
NumPy restatement (tests/exposure_ref.py), bit for bit; optim.ExponentialLR against its closed form; the argument checks of
appearance.Exposure and of train.trainStep's exposure / view pair that need no device."""
import math
import subprocess

import numpy as np
import pytest

import exposure_ref as ER
from common import host_program, run_host, same_bits

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program("exposure", tmp_path_factory.mktemp("exposure_host"))


def _run_host(host_exe, x, d, E, w=None):
    _, H, W = x.shape
    n = 3 * H * W
    arrays = [np.asarray(a, np.float32) for a in (E, x, d) + ((w,) if w is not None else ())]
    out, dx, terms = run_host(host_exe, [], np.array([W, H, int(w is not None)], np.int32).tobytes(), arrays,
                              [(np.float32, n), (np.float32, n), (np.float64, 12 * H * W)])
    return out.reshape(3, H, W), dx.reshape(3, H, W), terms.reshape(3, 4, H * W)


def _weights(W, H):
    """None, the random weight of the cases, and one of zeros and ones only"""
    rng = np.random.default_rng(W + 31 * H)
    return [None, ER.case(W, H, True)[3], (rng.random((H, W)) < 0.5).astype(np.float32)]


@pytest.mark.parametrize("W,H", [(1, 1), (5, 7), (67, 3), (129, 33)])
def test_header_statements_equal_the_restatement_bit_for_bit(host_exe, W, H):
    x, d, E, _ = ER.case(W, H, False)
    for w in _weights(W, H):
        out, dx, terms = _run_host(host_exe, x, d, E, w)
        assert same_bits(out, ER.forward(x, E, w))
        assert same_bits(dx, ER.backward_image(d, E, w))
        # float64(g) * float64(x), and g itself in column 3; the program reads a term off an accumulator that started at + 0: -0 comes as +0
        assert same_bits(terms, ER.terms(x, d, w) + 0.0)


@pytest.mark.parametrize("W,H", [(5, 7), (129, 33)])
def test_identity_row_returns_the_image_and_masks_exactly(host_exe, W, H):
    x, d, _, _ = ER.case(W, H, False)
    x.reshape(-1)[:3] = [-0.0, 0.0, np.float32(1e-45)]                       # a -0, a +0 and the smallest subnormal
    x.reshape(-1)[3:5] = [np.float32(3.4e38), np.float32(-3.4e38)]
    I = ER.identity()
    out, dx, _ = _run_host(host_exe, x, d, I, None)
    assert np.array_equal(out, x) and same_bits(out + np.float32(0), x + np.float32(0))      # the bits, but for -0 -> +0
    assert out.reshape(-1)[0] == 0 and not np.signbit(out.reshape(-1)[0])
    nz = x != 0
    assert same_bits(out[nz], x[nz])
    assert np.array_equal(dx, d)
    for w in _weights(W, H)[1:]:
        out, dx, _ = _run_host(host_exe, x, d, I, w)
        assert same_bits(out, w[None] * (x + np.float32(0)))                 # w * x exactly: masking a target needs no kernel of its own
        assert np.array_equal(out, w[None] * x)


def test_host_program_checks_itself_without_arguments(host_exe):
    """what `make -C tests sanitize-exposure` runs under ASan + UBSan: the built-in scene"""
    r = subprocess.run([host_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr


def test_restatement_of_the_exposure_gradient_is_the_float64_einsum():
    """the yardstick against itself: fsum of the exact terms against a plain float64 contraction, within the bound the device is held to"""
    x, d, E, w = ER.case(67, 3, True)
    dE, A = ER.backward_exposure(x, d, w)
    g = ER.weigh(d, w).astype(np.float64).reshape(3, -1)
    xa = np.concatenate([x.astype(np.float64).reshape(3, -1), np.ones((1, 67 * 3))])
    assert np.all(np.abs(g @ xa.T - dE) <= 67 * 3 * 2.0 ** -53 * A)
    assert np.all(A >= np.abs(dE)) and np.all(ER.dE_bound(dE, A, 67 * 3) > 0)


# ---------------------------------------------------------------- optim.ExponentialLR
def _close(a, b):
    return abs(a - b) <= 1e-15 * abs(b)


@pytest.mark.parametrize("a,b,n", [(0.01, 0.001, 30000), (1.6e-4, 1.6e-6, 30000), (0.5, 0.25, 7)])
def test_exponential_lr_closed_form(a, b, n):
    from gaussiansplat_amd.optim import ExponentialLR
    lr = ExponentialLR(a, b, n)
    assert _close(lr(0), a) and _close(lr(n), b)
    if n % 2 == 0:
        assert _close(lr(n // 2), math.sqrt(a * b))
    assert _close(lr(n / 2), math.sqrt(a * b))
    assert lr(2 * n) == lr(n) and lr(10 ** 9) == lr(n)                       # clipped beyond the end ...
    assert lr(-1) == 0.0 and lr(-10 ** 6) == 0.0                             # ... and 0 before the start
    for s in (1, n // 3, n - 1):
        t = s / n
        assert _close(lr(s), math.exp((1 - t) * math.log(a) + t * math.log(b)))
        assert b < lr(s) < a


def test_exponential_lr_delay():
    from gaussiansplat_amd.optim import ExponentialLR
    lr = ExponentialLR(0.01, 0.001, 1000, delay_steps=100, delay_mult=0.01)
    plain = ExponentialLR(0.01, 0.001, 1000)
    assert _close(lr(0), 0.01 * 0.01)                                        # sin(0) = 0: delay_mult itself
    assert _close(lr(100), plain(100)) and _close(lr(500), plain(500))       # sin(pi / 2) = 1 from delay_steps on
    assert _close(lr(50), plain(50) * (0.01 + 0.99 * math.sin(0.25 * math.pi)))
    assert ExponentialLR(0.0, 0.0, 10)(3) == 0.0
    for bad in (dict(lr_init=-1.0, lr_final=0.1, max_steps=5), dict(lr_init=0.1, lr_final=0.0, max_steps=5),
                dict(lr_init=0.1, lr_final=0.01, max_steps=0), dict(lr_init=0.1, lr_final=0.01, max_steps=5, delay_steps=-1),
                dict(lr_init=float("nan"), lr_final=0.01, max_steps=5)):
        with pytest.raises(ValueError):
            ExponentialLR(**bad)


# ---------------------------------------------------------------- appearance.Exposure / train.trainStep: argument checks (no GPU)
class _Stub:
    """what Exposure reads of a renderer before it touches a device: the image's shape"""
    def __init__(self, H=4, W=5):
        self.imageData = np.zeros((3, H, W), np.float32)


def test_exposure_argument_checks_raise_before_any_gpu_call():
    from gaussiansplat_amd.appearance import Exposure
    r = _Stub()
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            Exposure(r, bad)
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            Exposure(r, 2, lr=bad)
    with pytest.raises(ValueError):
        Exposure(r, 2, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        Exposure(r, 2, eps=0.0)
    with pytest.raises(ValueError):
        Exposure(r, 2, weights=[None])                                       # one entry per view
    with pytest.raises(ValueError):
        Exposure(r, 2, weights=[None, np.zeros((5, 4), np.float32)])         # [W, H] is not [H, W]
    with pytest.raises(ValueError):
        Exposure(r, 2, weights=[np.zeros((3, 4, 5), np.float32), None])


def test_exposure_view_checks_on_a_host_tensor():
    """a torch CPU tensor stands in for imageData: the object is built, and a view out of range is refused before any call into the library"""
    import torch
    from gaussiansplat_amd import train as TR
    from gaussiansplat_amd.appearance import Exposure

    class R:
        imageData = torch.zeros((3, 4, 5))
    e = Exposure(R(), 3, weights=[None, np.ones((4, 5), np.float32), None])
    assert tuple(e.table.shape) == (3, 3, 4) and np.array_equal(e.exposure(2), ER.identity()) and e.step_counts == [0, 0, 0]
    for bad in (-1, 3, 1.5, None, True):
        with pytest.raises(ValueError):
            e._view(bad)
        for call in (lambda: e.apply(bad, R.imageData), lambda: e.backward(bad, R.imageData), lambda: e.step(bad),
                     lambda: e.mask_target(bad, R.imageData), lambda: e.exposure(bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        e.apply(0, torch.zeros((3, 5, 4)))
    with pytest.raises(ValueError):
        e.set_lr(-1.0)
    gt = torch.zeros((3, 4, 5))
    assert e.mask_target(0, gt) is gt                                        # no weight: the target itself
    sd = e.state_dict()
    assert set(sd) == {"table", "exp_avg", "exp_avg_sq", "steps", "lr"} and sd["lr"] == 0.01
    sd["steps"] = [4, 0, 2]; sd["lr"] = 0.005
    e.load_state_dict(sd)
    assert e.step_counts == [4, 0, 2] and e.lr == 0.005
    with pytest.raises(ValueError):
        e.load_state_dict(dict(sd, steps=[1, 2]))
    # trainStep: the pair goes together, and the view is checked before anything is rendered (renderer None would fail at once otherwise)
    with pytest.raises(ValueError):
        TR.trainStep(None, gt, 0.1, None, exposure=e)
    with pytest.raises(ValueError):
        TR.trainStep(None, gt, 0.1, None, view=0)
    with pytest.raises(ValueError):
        TR.trainStep(None, gt, 0.1, None, exposure=e, view=3)
