"""The background colour on the host: train.RandomBackground is a seeded sequence of float32 colours, trainStep refuses what cannot work
before anything reaches the GPU, and the TWIN identity the GPU tests lean on holds on the oracle alone.

The twin: no colour is clamped anywhere (rgb = 0.5 + sum_k basis_k sh_k, basis_0 = 0.28209479177387814), and T = 1 - sum alpha_i T_i, so
    C + T bg = sum (c_i - bg) alpha_i T_i + bg
-- a render over bg is the black-background render of the scene whose degree-0 SH coefficients are lowered by bg / basis_0 per channel,
plus a constant.  Its gradients are therefore those of sum (C + T bg) . dC."""
import numpy as np
import pytest

from common import GRADS
from gaussiansplat_amd import train as TR

SH_C0 = 0.28209479177387814
BG = (1.0, 0.25, 0.6)


def test_random_background_is_a_seeded_float32_sequence():
    a, b, c = TR.RandomBackground(7), TR.RandomBackground(7), TR.RandomBackground(8)
    sa, sb, sc = ([x.draw() for _ in range(50)] for x in (a, b, c))
    assert sa == sb and sa != sc
    assert a.iteration == 50
    want = np.random.default_rng(7).random((50, 3), dtype=np.float32)       # three uniform float32 values per iteration, in order
    assert np.array_equal(np.asarray(sa, np.float64), want.astype(np.float64))
    for rgb in sa:
        assert len(rgb) == 3 and all(isinstance(x, float) and 0.0 <= x < 1.0 and float(np.float32(x)) == x for x in rgb)
    assert TR.RandomBackground().draw() == TR.RandomBackground(seed=0).draw()


def test_random_background_refuses_a_non_renderer_and_does_not_count_it():
    bg = TR.RandomBackground(1)
    with pytest.raises(ValueError, match="GaussianRenderer"):
        bg.apply(object())
    assert bg.iteration == 0
    assert bg.draw() == TR.RandomBackground(1).draw()                      # nothing was drawn for the refused call


@pytest.mark.parametrize("target", [np.zeros((3, 8, 8), np.float32), np.zeros((8, 8), np.float32), None], ids=["rgb", "plane", "none"])
def test_train_step_refuses_a_random_background_without_an_rgba_target(target):
    class Untouchable:                                                     # any use of the renderer or the loss would raise AttributeError
        pass
    bg = TR.RandomBackground(2)
    with pytest.raises(ValueError, match=r"4, H, W"):
        TR.trainStep(Untouchable(), target, 0.0, Untouchable(), background=bg)
    assert bg.iteration == 0                                               # a refused step is not counted


def test_oracle_twin_has_the_gradients_of_the_background_render(oracle):
    """O.backward on the DC-shifted twin against fp64 autograd of sum (img + trans * bg) . dC: rel-L2 <= 1e-5, the bar of
    tests/test_oracle_grad.py for oracle against autograd.  The twin's lists and transmittance are the scene's own, bit for bit, and the
    black-background gradients are far from the twin's -- so a background that is ignored cannot pass for one that is handled."""
    import torch

    import torch_ref
    from common import rel_l2, scene_and_cameras
    from gaussiansplat_amd import synthetic
    O = oracle
    n, W, H, deg, seed, order, t_min = 140, 48, 40, 1, 22, 0, 0.0
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, seed)
    args = lambda s: (s["means"], s["scales"], s["quats"], s["opacities"], s["shs"], deg, ocam)
    ref = O.render(*args(sc), order=order, t_min=t_min)
    dC = synthetic.make_dC(W, H, seed)
    twin = dict(sc)
    twin["shs"] = sc["shs"].copy()
    twin["shs"][:, 0, :] -= (np.asarray(BG, np.float64) / SH_C0).astype(np.float32)
    tref = O.render(*args(twin), order=order, t_min=t_min)
    assert np.array_equal(tref["ranges"], ref["ranges"]) and np.array_equal(tref["ids"], ref["ids"])
    assert np.array_equal(tref["trans"], ref["trans"])

    params = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in GRADS]
    img, trans = torch_ref.render(params, deg, T, P, float(cam.fx), float(cam.fy), cam.eye, cam.lookAt, float(np.float32(cam.near)),
                                  float(np.float32(cam.far)), W, H, ref["ranges"], ref["ids"], ref["pre"]["bbs"], ref["pre"]["tps"][:, 2],
                                  t_min=t_min)
    bg = torch.tensor(BG, dtype=torch.float64)
    ((img + trans[None] * bg[:, None, None]) * torch.tensor(dC, dtype=torch.float64)).sum().backward()
    g = O.backward(*args(twin), ref["ranges"], ref["ids"], dC, t_min=t_min)
    black = O.backward(*args(sc), ref["ranges"], ref["ids"], dC, t_min=t_min)
    for p, name in zip(params, GRADS):
        want = p.grad.numpy().reshape(-1)
        assert rel_l2(g[name].reshape(-1), want) <= 1e-5, (name, rel_l2(g[name].reshape(-1), want))
    assert rel_l2(black["means"].reshape(-1), g["means"].reshape(-1)) > 0.1
    assert rel_l2(black["shs"].reshape(-1), g["shs"].reshape(-1)) <= 1e-6   # d colour does not see the background
