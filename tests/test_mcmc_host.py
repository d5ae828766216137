"""MCMC densification without a GPU: the statements of csrc/gs_mcmc.h in a host build (tests/mcmc_host.cpp, built by tests/Makefile) against the
NumPy restatement (tests/mcmc_ref.py) -- weights, draws, noise and regulariser gradients bit for bit, the relocation within one float32 ulp --,
properties of the restatement itself, and the argument checks of gaussiansplat_amd.mcmc that need no device."""
import math
import subprocess

import numpy as np
import pytest

import mcmc_ref as M
from common import host_program, run_host, same_bits

f32 = np.float32
MIN_OPACITY = 0.005
MIN_LOGIT = f32(math.log(MIN_OPACITY / (1.0 - MIN_OPACITY)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program("mcmc", tmp_path_factory.mktemp("mcmc_host"))


def _run(host_exe, mode, n, head, arrays, outs):
    """head: packed scalars behind the int64 n; arrays: the inputs; outs: [(dtype, count)] of the outputs."""
    return run_host(host_exe, [mode], np.int64(n).tobytes() + head, arrays, outs)


def _edge_opacities():
    """random logits around the threshold, plus NaN, +-Inf, the threshold itself and its neighbours, and logits whose sigmoid rounds to 1"""
    rng = np.random.default_rng(5)
    o = rng.uniform(-9.0, 9.0, 4000).astype(f32)
    edge = [np.nan, np.inf, -np.inf, MIN_LOGIT, np.nextafter(MIN_LOGIT, f32(0)), np.nextafter(MIN_LOGIT, f32(-10)), 16.0, 16.7, 17.5, 25.0, 40.0, 88.0, 89.0,
            -87.0, -88.0, -104.0, 0.0, -0.0]
    o[:len(edge)] = np.array(edge, f32)
    return o


def test_weights_equal_the_restatement_bit_for_bit(host_exe):
    o = _edge_opacities()
    (w,) = _run(host_exe, "weight", len(o), f32(MIN_LOGIT).tobytes(), [o], [(np.uint32, len(o))])
    ref = M.weights(o, MIN_LOGIT)
    assert same_bits(w, ref)
    assert not w[:6][[0, 1, 2, 3, 5]].any() and w[4] > 0                     # NaN, +Inf (its sigmoid is NaN), -Inf, at and below the threshold: 0
    assert (w[8:12] == 2 ** 24).all() and w.max() == 2 ** 24                # a sigmoid that rounds to 1: the weight of one
    assert w[12] == 0                                                       # exp overflows: Inf / Inf


def test_draws_equal_searchsorted_bit_for_bit(host_exe):
    o = _edge_opacities()
    cdf, dead, (alive, ndead, total) = M.plan(o, MIN_LOGIT)
    assert alive + ndead == len(o) and total == int(M.weights(o, MIN_LOGIT).astype(np.uint64).sum()) and total > 2 ** 32
    rng = np.random.default_rng(6)
    u = rng.random(3000).astype(f32)
    edge = np.array([0.0, np.nextafter(f32(1), f32(0)), 1.0, -1.0, np.nan, -0.0, 2.0, np.inf, -np.inf, 1e-30], f32)
    # u landing exactly on CDF boundaries: the smallest float whose target reaches cdf[i], and its predecessor, for some i
    on = []
    for i in rng.integers(0, len(o) - 1, 200):
        x = f32(float(cdf[i]) / float(total))
        on += [x, np.nextafter(x, f32(0)), np.nextafter(x, f32(1))]
    u = np.concatenate([edge, np.array(on, f32), u])
    (src,) = _run(host_exe, "draw", len(o), np.int64(len(u)).tobytes(), [cdf, u], [(np.int32, len(u))])
    ref = M.sample(cdf, u)
    assert same_bits(src, ref)
    # every target of a small CDF whose total is a power of two: u = j / 2048 is exact, t = j -- every boundary is hit exactly, and then the
    # NEXT gaussian with a weight is taken
    ws = rng.integers(0, 4, 700).astype(np.uint64)
    ws[-1] = 2048 - int(ws[:-1].sum())
    small = np.cumsum(ws, dtype=np.uint64)
    us = (np.arange(2048) / 2048.0).astype(f32)
    (ss,) = _run(host_exe, "draw", len(small), np.int64(len(us)).tobytes(), [small, us], [(np.int32, len(us))])
    assert np.array_equal(M.targets(us, 2048), np.arange(2048, dtype=np.uint64)) and same_bits(ss, M.sample(small, us))
    assert same_bits(ss, np.repeat(np.arange(700), ws.astype(np.int64)).astype(np.int32))      # gaussian i owns exactly w[i] targets
    w = M.weights(o, MIN_LOGIT)
    assert (w[ref] > 0).all() and ref.min() >= 0 and ref.max() < len(o)       # a dead gaussian is never drawn
    assert ref[0] == ref[3] == ref[4] == ref[5] == np.flatnonzero(w)[0]       # 0, -1, NaN, -0: the first gaussian with a weight
    assert ref[1] == ref[2] == ref[6] == ref[7]                               # nextafter(1, 0), 1, 2, Inf: one place


def test_noise_equals_the_restatement_bit_for_bit(host_exe):
    rng = np.random.default_rng(7)
    n = 3000
    means = rng.normal(0, 2, (n, 3)).astype(f32)
    scales = rng.uniform(-7.0, -1.0, (n, 3)).astype(f32)
    quats = rng.normal(0, 1, (n, 4)).astype(f32) * rng.uniform(0.2, 3.0, (n, 1)).astype(f32)     # raw: not normalised
    opac = rng.uniform(-9.0, 4.0, n).astype(f32)
    opac[:6] = np.array([MIN_LOGIT, np.nextafter(MIN_LOGIT, f32(0)), np.nextafter(MIN_LOGIT, f32(-10)), -5.0, -5.6, np.nan], f32)   # sig on both sides of gate_t
    z = rng.normal(0, 1, (n, 3)).astype(f32)
    z[10:20] = 0.0
    scales[20] = 60.0                                                       # exp(2 * 60) overflows: the mean is kept
    z[21] = np.inf
    for lr, gk, gt in ((80.0, 100.0, 0.005), (1e-3, 100.0, 0.005), (5.0, 0.0, 0.5)):
        (out,) = _run(host_exe, "noise", n, np.array([lr, gk, gt], f32).tobytes(), [means, scales, quats, opac, z], [(f32, 3 * n)])
        ref = M.noise(means, scales, quats, opac, z, lr, gk, gt)
        assert same_bits(out.reshape(n, 3), ref)
        assert same_bits(ref[[5, 20, 21]], means[[5, 20, 21]]) and np.array_equal(ref[10:20], means[10:20])
        assert (ref != means).any(axis=1).sum() > n // 2 or lr < 1e-2


def test_regulariser_gradients_equal_the_restatement_bit_for_bit(host_exe):
    rng = np.random.default_rng(8)
    n = 3000
    opac = _edge_opacities()[:n]
    scales = rng.uniform(-9.0, 2.0, (n, 3)).astype(f32)
    d_op = rng.normal(0, 1e-4, n).astype(f32)
    d_sc = rng.normal(0, 1e-4, (n, 3)).astype(f32)
    c_o, c_s = M.reg_coefficients(0.01, 0.01, n)
    assert c_o == f32(0.01 / n) and c_s == f32(0.01 / (3 * n))
    out_o, out_s = _run(host_exe, "reg", n, np.array([c_o, c_s], f32).tobytes(), [opac, scales, d_op, d_sc], [(f32, n), (f32, 3 * n)])
    ref_o, ref_s = M.regularize(d_op, d_sc, opac, scales, c_o, c_s)
    nan = np.isnan(ref_o)
    assert np.array_equal(nan, np.isnan(out_o)) and same_bits(out_o[~nan], ref_o[~nan]) and same_bits(out_s.reshape(n, 3), ref_s)
    assert (ref_o[~nan] >= d_op[~nan]).all() and (ref_s > d_sc).any()


def _relocation_grid():
    """o over [0.0051, 1 - 2^-23] as float32 logits x every n in 2..51 (count c = n - 1), and the counts beyond the table"""
    o = np.concatenate([np.geomspace(0.0051, 0.5, 60), 1.0 - np.geomspace(0.5, 2.0 ** -23, 60), [0.0051, 1.0 - 2.0 ** -23, 0.5, 0.99, 0.999999]])
    logit = np.log(o / (1.0 - o)).astype(f32)
    logit[len(o) - 4] = np.nextafter(f32(np.log((1.0 - 2.0 ** -23) / 2.0 ** -23)), f32(0))
    cs = np.concatenate([np.arange(1, 51), [51, 52, 100, 200, 10 ** 6]])
    L, Cc = np.meshgrid(logit, cs, indexing="ij")
    rng = np.random.default_rng(9)
    return L.reshape(-1).astype(f32), Cc.reshape(-1).astype(np.int32), rng.uniform(-7.0, 0.0, (L.size, 3)).astype(f32)


def test_relocation_within_one_float_ulp_of_the_restatement(host_exe):
    """Both sides evaluate in double to <= 1e-12 relative and round to float once: they can differ only where the double value sits next to a
    float rounding boundary, by one ulp of the reference value.  Every o of the grid, every n in 2..51: no case left out."""
    opac, c, scales = _relocation_grid()
    n = len(opac)
    sig = M.sigmoid(opac).astype(np.float64)
    assert sig.min() <= 0.0051 * (1 + 1e-6) and sig.max() >= 1.0 - 2.0 ** -23 and set(range(1, 51)) <= set(c.tolist())
    op, sc = _run(host_exe, "relocate", n, f32(MIN_OPACITY).tobytes(), [opac, scales, c], [(f32, n), (f32, 3 * n)])
    ref_op, ref_sc = M.relocate_values(opac, scales, c, MIN_OPACITY)
    assert np.isfinite(ref_op).all() and np.isfinite(ref_sc).all()
    d_op = np.abs(op.astype(np.float64) - ref_op.astype(np.float64))
    d_sc = np.abs(sc.reshape(n, 3).astype(np.float64) - ref_sc.astype(np.float64))
    print("relocation: %d of %d opacities and %d of %d scales differ from the restatement, largest %.3g / %.3g ulp"
          % ((d_op > 0).sum(), n, (d_sc > 0).sum(), 3 * n, (d_op / np.spacing(np.abs(ref_op))).max(), (d_sc / np.spacing(np.abs(ref_sc))).max()))
    assert (d_op <= np.spacing(np.abs(ref_op))).all()
    assert (d_sc <= np.spacing(np.abs(ref_sc))).all()


def test_host_program_checks_itself_without_arguments(host_exe):
    """what `make -C tests sanitize-mcmc` runs under ASan + UBSan: the built-in scene"""
    r = subprocess.run([host_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- properties of the restatement itself
def test_relocated_opacity_composes_back_to_the_source():
    """n copies of opacity p render like one of opacity o: 1 - (1 - p)^n = o"""
    o = np.concatenate([np.geomspace(0.0051, 0.5, 40), 1.0 - np.geomspace(0.5, 2.0 ** -23, 40)])
    for n in range(2, 52):
        p = M.relocate_p(o, n)
        back = -np.expm1(n * np.log1p(-p))
        assert np.all(np.abs(back - o) <= 1e-12), n
        assert np.all((p > 0) & (p < o))


def test_relocate_leaves_everything_else_untouched_and_clamps():
    rng = np.random.default_rng(10)
    n, k3 = 400, 12
    model = [rng.normal(0, 1, (n, 3)).astype(f32), rng.uniform(-6, -1, (n, 3)).astype(f32), rng.normal(0, 1, (n, 4)).astype(f32),
             rng.uniform(-4.0, 6.0, (n, 1)).astype(f32), rng.normal(0, 1, (n, k3)).astype(f32)]
    model[3][7, 0] = f32(math.log(0.0052 / 0.9948))                          # barely alive: its copies clamp at min_opacity
    sets = [[rng.normal(0, 1, x.shape).astype(f32) for x in model], [None, rng.normal(0, 1, (n, 3)).astype(f32), None, None, None]]
    src = np.array([5] * 1 + [6] * 2 + [7] * 20 + [8] * 50 + [9] * 51 + [10] * 200 + [-1, n, 11], np.int64)
    dst = np.concatenate([np.arange(20, 20 + len(src) - 3), [12, 13, n + 5]])
    new, new_sets, cnt = M.relocate(model, src, dst, MIN_OPACITY, sets)
    assert cnt[5] == 1 and cnt[10] == 200 and cnt[11] == 0 and cnt.sum() == len(src) - 3            # out-of-range entries are not counted
    touched = np.zeros(n, bool)
    touched[[5, 6, 7, 8, 9, 10]] = True
    touched[dst[:-3]] = True
    for a, b in zip(model, new):                                             # c = 0 sources and everything else: every bit
        assert same_bits(a[~touched], b[~touched])
    for i in (0, 2, 4):                                                      # sources keep means, quaternions, SH rows
        assert same_bits(model[i][5:11], new[i][5:11])
    assert same_bits(new[0][dst[:-3]], model[0][src[:-3]]) and same_bits(new[4][dst[:-3]], model[4][src[:-3]])
    assert (new[3][5:11, 0] < model[3][5:11, 0]).all() and (new[1][5:11] < model[1][5:11]).all()
    assert new[3][7, 0] == f32(math.log(float(f32(MIN_OPACITY))) - math.log1p(-float(f32(MIN_OPACITY))))   # the clamp engages at min_opacity
    assert same_bits(new[3][dst[3:23], 0], np.full(20, new[3][7, 0], f32))
    # a draw count above 50 equals the count-50 result
    a = M.relocate_values(model[3][8:11, 0], model[1][8:11], [50, 50, 50], MIN_OPACITY)
    b = M.relocate_values(model[3][8:11, 0], model[1][8:11], [50, 51, 200], MIN_OPACITY)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    for s_old, s_new in zip(sets, new_sets):
        for x, y in zip(s_old, s_new):
            if x is None:
                assert y is None
                continue
            assert not y[touched].any() and not np.signbit(y[touched]).any() and same_bits(x[~touched], y[~touched])


# ---------------------------------------------------------------- gaussiansplat_amd.mcmc: argument checks (no GPU)
def test_controller_argument_checks_raise_before_any_gpu_call():
    from gaussiansplat_amd import mcmc
    ok = dict(cap_max=1000)
    c = mcmc.MCMCController(**ok)
    assert (c.from_iter, c.until_iter, c.interval, c.noise_lr, c.growth) == (500, 25000, 100, 5e5, 1.05)
    assert c.refine_due(500) and c.refine_due(25000) and not c.refine_due(499) and not c.refine_due(550) and not c.refine_due(25100)
    for bad in (dict(cap_max=0), dict(cap_max=1.5), dict(cap_max=True), dict(cap_max=10, interval=0), dict(cap_max=10, from_iter=-1),
                dict(cap_max=10, from_iter=10, until_iter=5), dict(cap_max=10, min_opacity=0.0), dict(cap_max=10, min_opacity=1.0),
                dict(cap_max=10, opacity_reg=-1.0), dict(cap_max=10, scale_reg=float("nan")), dict(cap_max=10, growth=0.9),
                dict(cap_max=10, noise_lr=float("inf")), dict(cap_max=10, means_lr=-1.0)):
        with pytest.raises(ValueError):
            mcmc.MCMCController(**bad)
    with pytest.raises(ValueError):                                          # neither an optimiser nor means_lr: the noise has no rate
        c.after_step(object(), None)
    assert c.iteration == 0
    for call in (lambda: mcmc.relocate(object()), lambda: mcmc.grow(object(), cap_max=10), lambda: mcmc.inject_noise(object(), 1.0),
                 lambda: mcmc.regularize(object())):
        with pytest.raises(ValueError):                                      # not the 3-D renderer
            call()
