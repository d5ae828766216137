"""Density control without a GPU: invariants of the NumPy reference (tests/density_ref.py) the device is compared against, the schedule
of density.DensityController and the host-side validation of its arguments and of the thresholds."""
import math

import numpy as np
import pytest

import density_ref as D
from common import same_bits

f32 = np.float32


def _model(rng, n, k3):
    return [rng.standard_normal((n, w)).astype(f32) for w in (3, 3, 4, 1, k3)]


@pytest.mark.parametrize("n", [0, 1, 7, 300])
def test_counts_add_up_and_n_out_formula(n):
    rng = np.random.default_rng(n)
    action = rng.integers(0, 4, n).astype(np.int32)
    c = D.counts(action)
    assert c[0] + c[2] + c[3] == n                              # survivors (keep + clone sources), split sources, pruned
    assert c[1] <= c[0]
    model, noise = _model(rng, n, 12), rng.standard_normal((n, 2, 3)).astype(f32)
    sets = [_model(rng, n, 12), _model(rng, n, 12)]
    sets[1][2] = None
    new, new_sets = D.restructure(model, action, noise, sets=sets)
    assert all(a.shape == (D.n_out(c), w) for a, w in zip(new, (3, 3, 4, 1, 12)))
    assert new_sets[1][2] is None
    for s in new_sets:
        for a, src in zip(s, sets[0]):
            if a is not None:
                assert a.shape[0] == D.n_out(c) and not a[c[0]:].any() and not np.signbit(a[c[0]:]).any()   # new rows are +0


def test_all_keep_is_the_identity_and_all_prune_is_empty():
    rng = np.random.default_rng(5)
    n = 257
    model = _model(rng, n, 48)
    model[0][3, 1] = np.nan                                     # a NaN travels bit for bit
    sets = [_model(rng, n, 48)]
    new, new_sets = D.restructure(model, np.zeros(n, np.int32), None, sets=sets)
    for a, b in zip(new + new_sets[0], model + sets[0]):
        assert same_bits(a, b)
    new, new_sets = D.restructure(model, np.full(n, 3, np.int32), None, sets=sets)
    assert all(a.shape[0] == 0 for a in new + new_sets[0])


def test_rows_are_ordered_survivors_clones_children():
    rng = np.random.default_rng(6)
    n = 64
    model = _model(rng, n, 3)
    model[3][:, 0] = np.arange(n, dtype=f32)                    # the opacity column names the source row
    action = rng.integers(0, 4, n).astype(np.int32)
    noise = rng.standard_normal((n, 2, 3)).astype(f32)
    new, _ = D.restructure(model, action, noise, log_shrink=f32(0.25))
    surv, cl, sp = np.flatnonzero(action <= 1), np.flatnonzero(action == 1), np.flatnonzero(action == 2)
    assert np.array_equal(new[3][:, 0], np.concatenate([surv, cl, np.repeat(sp, 2)]).astype(f32))
    kids = slice(len(surv) + len(cl), None)
    assert same_bits(new[1][kids], np.repeat(model[1][sp] - f32(0.25), 2, axis=0))
    assert same_bits(new[2][kids], np.repeat(model[2][sp], 2, axis=0))
    # a child sits at mean + R diag(exp(scale)) z: with z = 0 it sits on its source
    new0, _ = D.restructure(model, action, np.zeros((n, 2, 3), f32))
    assert np.array_equal(new0[0][kids], np.repeat(model[0][sp], 2, axis=0))
    # the rotation is the preprocess's: identity for the unit quaternion
    assert np.array_equal(D.quat_to_rot(np.array([[1, 0, 0, 0]], f32))[0], np.eye(3, dtype=f32))


def test_decide_thresholds_are_exact_and_nan_is_kept():
    thr, lss, ls, mo, mw, px = f32(2e-4), f32(-3.0), f32(0.5), f32(-2.0), f32(-1.0), 20
    #             grad_sum          count  ext  smax   opacity   expected
    rows = [(f32(thr * f32(3)),      3,     0,  -3.5,   0.0,     1),      # on the gradient threshold: densified (>=); small: clone
            (np.nextafter(f32(thr * f32(3)), f32(0)), 3, 0, -3.5, 0.0, 0),   # one ulp below: kept
            (f32(1.0),               0,     0,  -3.5,   0.0,     0),      # never visible: kept
            (f32(1.0),               2,     0,  -3.0,   0.0,     1),      # on the split scale: not above it -> clone
            (f32(1.0),               2,     0,  -2.9,   0.0,     2),      # above: split
            (f32(0.0),               2,     0,  -3.5,  -2.0,     0),      # on the opacity threshold: not below it -> kept
            (f32(0.0),               2,     0,  -3.5,  -2.1,     3),
            (f32(0.0),               2,    20,  -3.5,   0.0,     0),      # on the extent threshold: not above it
            (f32(0.0),               2,    21,  -3.5,   0.0,     3),
            (f32(0.0),               2,     0,  -1.0,   0.0,     0),      # on the world-scale threshold
            (f32(0.0),               2,     0,  -0.9,   0.0,     3),
            (f32(1.0),               2,     0,  -0.6,   0.0,     2),      # split: what remains is -1.1 <= -1 -> survives as a split
            (f32(1.0),               2,     0,  -0.4,   0.0,     3),      # ... remains -0.9: pruned (prune wins over densify)
            (f32(np.nan),            2,     0,  -3.5,   0.0,     0),      # NaN statistics: kept
            (f32(1.0),               2,     0, np.nan,  0.0,     1),      # NaN scale: densified by its gradient, every scale test false -> clone
            (f32(0.0),               2,     0,  -3.5, np.nan,    0)]      # NaN opacity: kept
    gs = np.array([r[0] for r in rows], f32)
    cnt = np.array([r[1] for r in rows], np.int32)
    ext = np.array([r[2] for r in rows], np.int32)
    scales = np.stack([np.array([r[3] for r in rows], f32), np.full(len(rows), -6.0, f32), np.full(len(rows), -7.0, f32)], axis=1)
    opac = np.array([r[4] for r in rows], f32)
    got = D.decide(scales, opac, gs, cnt, ext, thr, lss, ls, mo, mw, px)
    assert got.tolist() == [r[5] for r in rows]
    off = D.decide(scales, opac, gs, cnt, ext, thr, lss, ls, mo, f32(np.inf), 0)      # +Inf and 0 switch the two tests off
    assert off[8] == 0 and off[10] == 0 and off[12] == 2


def test_opacity_reset_reference():
    o = np.array([[-6.0], [5.0], [np.nan], [-4.59512], [np.inf]], f32)
    out, m, v = D.opacity_reset(o, f32(-4.59512), np.ones((5, 1), f32), None)
    assert same_bits(out, np.array([[-6.0], [-4.59512], [np.nan], [-4.59512], [-4.59512]], f32))
    assert v is None and not m.any()


def test_accumulate_reference_visibility():
    W, H = 200, 136
    bbs = np.array([[10, 20, 30, 25], [1, 1, 0, 5], [5, 5, 5, 5], [np.nan, 1, 2, 3], [10, 20, 30, 25], [10, 20, 30, 25]], f32)
    tps = np.zeros((6, 4), f32); tps[:, 2] = 30.0; tps[4, 2] = 200.0
    rgb, sig, mu, inv = np.ones((6, 3), f32), np.full(6, 0.5, f32), np.ones((6, 2), f32), np.ones((6, 4), f32)
    sig[5] = np.inf
    vis, ext = D.visibility(bbs, tps, rgb, sig, mu, inv, 0.1, 100.0)
    assert vis.tolist() == [True, False, True, False, False, False] and ext.tolist() == [21, 0, 1, 0, 0, 0]
    g = np.zeros((6, 10), f32); g[:, 4] = 3e-3; g[:, 5] = -4e-3
    gs, cnt, mx = D.accumulate(np.zeros(6, f32), np.zeros(6, np.int32), np.full(6, 7, np.int32), g, W, H, vis, ext)
    a, b = f32(100.0) * f32(3e-3), f32(68.0) * f32(-4e-3)
    assert same_bits(gs, np.full(6, np.sqrt(f32(a * a + b * b)), f32))
    assert cnt.tolist() == [1, 0, 1, 0, 0, 0] and mx.tolist() == [21, 7, 7, 7, 7, 7]


# ---------------------------------------------------------------- the controller and the thresholds (host-side validation)
def test_controller_schedule_defaults_are_the_papers():
    from gaussiansplat_amd.density import DensityController
    c = DensityController(scene_extent=5.0)
    assert (c.from_iter, c.until_iter, c.interval, c.opacity_reset_interval) == (500, 15000, 100, 3000)
    due = [it for it in range(1, 16001) if c.densify_due(it)]
    assert due[0] == 500 and due[1] == 600 and due[-1] == 15000 and len(due) == 146
    assert [it for it in range(1, 16001) if c.reset_due(it)] == [3000, 6000, 9000, 12000, 15000]
    assert c.wants_stats(1) and c.wants_stats(15000) and not c.wants_stats(15001) and not c.wants_stats(0)


def test_controller_schedule_custom():
    from gaussiansplat_amd.density import DensityController
    c = DensityController(scene_extent=1.0, from_iter=5, until_iter=26, interval=10, opacity_reset_interval=0)
    assert [it for it in range(0, 40) if c.densify_due(it)] == [10, 20]
    assert not any(c.reset_due(it) for it in range(0, 40))
    c = DensityController(scene_extent=1.0, from_iter=0, until_iter=30, interval=7, opacity_reset_interval=15)
    assert [it for it in range(0, 40) if c.densify_due(it)] == [7, 14, 21, 28]
    assert [it for it in range(0, 40) if c.reset_due(it)] == [15, 30]


@pytest.mark.parametrize("kw", [dict(scene_extent=0.0), dict(scene_extent=-1.0), dict(scene_extent=math.nan), dict(scene_extent=math.inf),
                                dict(scene_extent="big"), dict(from_iter=-1), dict(interval=0), dict(interval=2.5), dict(until_iter=10, from_iter=20),
                                dict(opacity_reset_interval=-3), dict(grad_threshold=-1e-4), dict(grad_threshold=math.nan),
                                dict(percent_dense=0.0), dict(min_opacity=0.0), dict(min_opacity=1.0), dict(max_world_fraction=0.0),
                                dict(max_world_fraction=-0.1), dict(max_extent_px=-1), dict(reset_opacity_to=0.0), dict(reset_opacity_to=1.5),
                                dict(max_gaussians=0), dict(max_gaussians=2.5), dict(interval=True)])
def test_controller_refuses_bad_arguments(kw):
    from gaussiansplat_amd.density import DensityController
    with pytest.raises(ValueError):
        DensityController(**{"scene_extent": 5.0, **kw})


def test_thresholds_are_converted_to_log_and_logit_space():
    import ctypes as C
    from gaussiansplat_amd import backend as B
    from gaussiansplat_amd.density import density_params
    p = density_params(scene_extent=4.0, grad_threshold=2e-4, percent_dense=0.01, min_opacity=0.005, max_world_fraction=0.1, max_extent_px=20)
    assert p.struct_size == C.sizeof(B.GsDensityParams) == 28
    assert p.grad_threshold == f32(2e-4) and p.log_split_scale == f32(math.log(0.04)) and p.log_shrink == f32(math.log(1.6))
    assert p.min_opacity_logit == f32(math.log(0.005 / 0.995)) and p.log_max_world_scale == f32(math.log(0.4)) and p.max_extent_px == 20
    assert D.LOG_SHRINK_3DGS == f32(p.log_shrink)
    q = density_params(scene_extent=4.0, grad_threshold=math.inf, max_world_fraction=None)
    assert q.grad_threshold == math.inf and q.log_max_world_scale == math.inf and q.max_extent_px == 0


def test_train_step_refuses_density_with_the_fused_forms():
    from gaussiansplat_amd import train as TR
    from gaussiansplat_amd.density import DensityController

    class FusedOpt:
        fused = True
    c = DensityController(scene_extent=1.0)
    with pytest.raises(ValueError, match="unfused"):
        TR.trainStep(None, None, 0.0, None, optimizer=FusedOpt(), density=c)
    with pytest.raises(ValueError, match="unfused"):
        TR.trainStep(None, None, 0.0, None, fused_sgd=True, density=c)


def test_header_density_structs_match_the_python_mirror():
    """gs_density_stats / gs_density_params of include/gsplat.h, field for field, against backend.GsDensityStats / GsDensityParams."""
    import os
    import re
    from gaussiansplat_amd import backend as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gsplat.h")).read(), flags=re.S)
    for cname, cls in (("gs_density_stats", B.GsDensityStats), ("gs_density_params", B.GsDensityParams)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + cname + r"\s*;", src).group(1)
        names = [re.fullmatch(r"[A-Za-z_0-9]+\s*\*?\s*([A-Za-z_0-9]+)", f.strip()).group(1) for f in body.split(";") if f.strip()]
        assert names == [f[0] for f in cls._fields_], cname
