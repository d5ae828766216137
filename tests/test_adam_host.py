"""Adam without a GPU: the NumPy restatement of include/gsplat.h's arithmetic against torch.optim.Adam, optim.Adam's argument
checks and its state_dict round trip (the device steps are tests/test_gpu_adam.py)."""

import numpy as np
import pytest

import adam_ref as A

BETAS = (0.9, 0.999)
LR6 = (1e-3, 5e-3, 2e-3, 5e-2, 2.5e-3, 1.25e-4)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("eps", [1e-8, 1e-15])
def test_restatement_matches_torch_adam_per_group(eps):
    """Each of the six groups over 20 steps (the SH columns as two runs, as torch must treat them) within 1e-6 relative."""
    rng = np.random.default_rng(5)
    n, k3 = 97, 48
    widths = (3, 3, 4, 1, k3)
    params = [rng.standard_normal((n, w)).astype(np.float32) for w in widths]
    m = [np.zeros((n, w), np.float32) for w in widths]
    v = [np.zeros((n, w), np.float32) for w in widths]
    seq = []
    for t in range(1, 21):
        g = [(rng.standard_normal((n, w)) * 10.0 ** rng.uniform(-4, 1)).astype(np.float32) for w in widths]
        for a in g:
            a[rng.random(a.shape) < 0.1] = 0.0
        seq.append(g)
    p0 = [a.copy() for a in params]
    for t, g in enumerate(seq, 1):
        params, m, v = A.step(params, g, m, v, LR6, *BETAS, eps, t)
    for k in range(5):
        cols = [slice(None)] if k < 4 else [slice(0, 3), slice(3, None)]
        for j, cs in enumerate(cols):
            grp = k if k < 4 else 4 + j
            tp, tm, tv = A.torch_adam(p0[k][:, cs], [g[k][:, cs] for g in seq], LR6[grp], BETAS, eps)
            for got, want in ((params[k][:, cs], tp), (m[k][:, cs], tm), (v[k][:, cs], tv)):
                assert _rel(got, want) <= 1e-6, (grp, _rel(got, want))


def test_restatement_scalars_and_selective_rows():
    h = A.hyper(LR6, 0.9, 0.999, 1e-8, 3)
    assert h["omb1"] == np.float32(1.0 - float(np.float32(0.9)))
    assert h["step_size"][0] == np.float32(np.float32(1e-3) / (1.0 - float(np.float32(0.9)) ** 3))
    n = 8
    p = [np.ones((n, w), np.float32) for w in (3, 3, 4, 1, 3)]
    g = [np.zeros((n, w), np.float32) for w in (3, 3, 4, 1, 3)]
    g[4][1, 2] = -0.0
    g[0][2, 0] = 1.0
    g[3][3, 0] = np.nan
    zeros = [np.zeros_like(a) for a in p]
    P, M, V = A.step(p, g, zeros, zeros, LR6, 0.9, 0.999, 1e-8, 1, selective=True)
    live = [r for r in range(n) if not np.array_equal(P[0][r], p[0][r]) or np.any(M[3][r] != 0) or np.isnan(P[3][r]).any()]
    assert live == [2, 3]                                    # -0 is dead, NaN is live


class _FakeRenderer:
    """What optim.Adam reads from a renderer before any device call: the gradient buffer's layout."""

    def __init__(self, n=10, k3=12):
        import torch
        from gaussiansplat_amd import renderer as R
        d = R.SplatData3D(means=torch.zeros(n, 3), scales=torch.zeros(n, 3), shs=torch.zeros(n, k3), quaternions=torch.zeros(n, 4),
                          opacities=torch.zeros(n, 1))
        self._splatGrads = R.initGrads(d)


def test_optim_adam_argument_checks():
    from gaussiansplat_amd.optim import Adam
    r = _FakeRenderer()
    with pytest.raises(ValueError, match="unknown parameter groups"):
        Adam(r, lr={"means": 1e-3, "colour": 1.0, "scales": 1, "quaternions": 1, "opacities": 1, "sh_dc": 1, "sh_rest": 1})
    with pytest.raises(ValueError, match="no rate"):
        Adam(r, lr={"means": 1e-3})
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Adam(r, lr=bad)
        with pytest.raises(ValueError):
            Adam(r, lr=dict(means=1e-3, scales=1e-3, quaternions=bad, opacities=1e-3, sh_dc=1e-3, sh_rest=1e-3))
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.9), (float("nan"), 0.9)):
        with pytest.raises(ValueError, match="betas"):
            Adam(r, lr=1e-3, betas=betas)
    for eps in (0.0, -1e-8, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            Adam(r, lr=1e-3, eps=eps)
    opt = Adam(r, lr=1e-3)
    with pytest.raises(ValueError):
        opt.set_lr(shs=1e-3)
    with pytest.raises(ValueError):
        opt.set_lr(means=-1.0)
    opt.set_lr(means=2e-4)                                    # the 3DGS position-rate decay changes one rate between steps
    assert opt.lr_vector() == [2e-4, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3]


def test_optim_adam_for_3dgs_defaults():
    from gaussiansplat_amd.optim import Adam
    opt = Adam.for_3dgs(_FakeRenderer(), scene_extent=5.0)
    assert opt.lr_vector() == pytest.approx([8e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 1.25e-4])
    assert opt.eps == 1e-15 and opt.betas == (0.9, 0.999) and not opt.fused and not opt.selective


def test_optim_adam_state_dict_round_trip():
    import torch
    from gaussiansplat_amd.optim import Adam
    r = _FakeRenderer(n=10, k3=12)
    a = Adam(r, lr=1e-3, betas=(0.8, 0.99), eps=1e-10, selective=True)
    a.exp_avg.copy_(torch.arange(a.exp_avg.numel(), dtype=torch.float32))
    a.exp_avg_sq.copy_(torch.arange(a.exp_avg.numel(), dtype=torch.float32) * 0.5)
    a.step_count = 7
    a.set_lr(sh_rest=3e-5)
    sd = a.state_dict()
    b = Adam(_FakeRenderer(n=10, k3=12), lr=1.0)
    b.load_state_dict(sd)
    assert b.step_count == 7 and b.lr == a.lr and b.betas == (0.8, 0.99) and b.eps == 1e-10 and b.selective
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    a.exp_avg.zero_()                                         # the state dict holds copies
    assert not torch.equal(sd["exp_avg"], a.exp_avg)
    with pytest.raises(ValueError):
        Adam(_FakeRenderer(n=11, k3=12), lr=1.0).load_state_dict(sd)
