"""The per-gaussian reference of the composite backward (oracle.composite_rows, its fp32 twin, oracle.chain) on the CPU.

What test_gpu_pergaussian.py relies on is pinned here without a GPU: the new adjoint is the old one when both take the fp64 forward's
payload; the mass vanishes exactly where nothing contributes; the chain reproduces gso_backward's parameter gradients; a correct fp32
evaluation (the twin: the kernel's formulation in float) stays inside KAPPA_REF * 2^-24 * mass + floor on every touched gaussian of every
scene the GPU tests use (but the large heavy-tailed one) -- the measured kappa is printed per scene -- and the bound at KAPPA_TEST is tight enough to mean something.
"""
import numpy as np
import pytest

import pergaussian_ref as PR

CASES = [(name, t) for name in PR.SCENES if name not in PR.HEAVY for t in ((0.0, 1e-5, 0.2) if name == "dense" else (0.0, 1e-5))]
SCENES_3D = [k for k, v in PR.SCENES.items() if v[0] not in ("2d", "clustered")]      # (the heavy-tailed scene: composite cases only, it is large)


def _convert64(rows, f):
    """raw moments -> d{sig, mu, conic} with the fp64 sig and conic (what gso_backward's g2d holds)"""
    M = f["M"]; mc = 0.5 * (M[:, 1] + M[:, 2])
    g = np.zeros_like(rows)
    g[:, :3] = rows[:, :3]
    g[:, 3] = -rows[:, 3] / f["sig"]
    g[:, 4] = -(M[:, 0] * rows[:, 4] + mc * rows[:, 5])
    g[:, 5] = -(mc * rows[:, 4] + M[:, 3] * rows[:, 5])
    g[:, 6] = 0.5 * rows[:, 6]; g[:, 7] = g[:, 8] = 0.5 * rows[:, 7]; g[:, 9] = 0.5 * rows[:, 9]
    return g


@pytest.mark.parametrize("name", SCENES_3D)
@pytest.mark.parametrize("t_min", [0.0, 1e-5])
def test_rows_at_the_fp64_payload_are_gso_backward(oracle, name, t_min):
    """Same walk, same decisions, same payload: the new adjoint equals gso_backward's g2d to 1e-12 of the absolute-valued sums
    (the two add the pixels in different orders; mass / 8 bounds sum |term|, every weight being at least 8)."""
    O = oracle
    s = PR.scene(name); sc = s["sc"]; r = PR.reference(name, t_min)
    args = (sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], s["deg"], s["ocam"])
    gref = O.backward(*args, r["ranges"], r["ids"], s["dC"], t_min=t_min, omp=True)
    f = O.forward64(*args)
    got = O.composite_rows(f, r["pre"]["bbs"], r["pre"]["tps"], r["ranges"], r["ids"], s["ocam"], s["dC"], t_min=t_min, omp=True)
    conv = _convert64(got["rows"], f)
    scale = _convert64(got["mass"] / 8.0, dict(M=np.abs(f["M"]), sig=-f["sig"]))       # absolute-valued sums through the same step
    scale[:, 4:6] = np.abs(scale[:, 4:6])
    # (+ 1e-300: sums of fp64 subnormals, 1e-315 and below, carry no relative precision)
    assert np.all(np.abs(conv - gref["g2d"]) <= 1e-12 * (np.abs(gref["g2d"]) + np.abs(scale)) + 1e-300), np.abs(conv - gref["g2d"]).max()
    # the chain on gso_backward's own rows is gso_backward; on the raw rows it is the same to rounding
    again = O.chain(*args, gref["g2d"], raw=False)
    raw = O.chain(*args, got["rows"], raw=True)
    for k in ("means", "scales", "quats", "opacities", "shs"):
        assert np.array_equal(again[k], gref[k]), k
        assert np.linalg.norm(raw[k] - gref[k]) <= 1e-10 * np.linalg.norm(gref[k]), k


@pytest.mark.parametrize("name,t_min", CASES)
def test_mass_is_zero_exactly_where_no_pixel_contributes(oracle, name, t_min):
    r = PR.reference(name, t_min)
    tch = PR.touched(r)
    used = PR.ROW_USED
    assert 0 < tch.sum() <= len(tch)
    assert np.all((r["mass"][tch][:, :3] > 0).all(axis=1))                       # a touched gaussian has mass in every colour word
    for k in ("mass", "rows", "dropped", "floor"):
        assert np.all(r[k][~tch] == 0.0), k
        assert np.isfinite(r[k]).all(), k
        assert np.all(r[k][:, 8] == 0.0), k
    assert np.all(r["mass"][:, used] >= 0) and np.all(r["dropped"] >= 0)
    # the fp32 twin leaves those rows untouched too
    tw = PR.twin(name, t_min)
    assert np.all(tw[~tch] == 0.0) and np.isfinite(tw).all()


@pytest.mark.parametrize("name,t_min", CASES)
def test_twin_stays_inside_kappa_ref(oracle, name, t_min):
    """A correct fp32 evaluation of the adjoint, in the kernel's formulation, uses at most KAPPA_REF of the mass."""
    r = PR.reference(name, t_min)
    k, where = PR.kappa_of(PR.twin(name, t_min), r)
    print(f"\nkappa_ref[{name}, t_min={t_min:g}] = {k:.3f} at gaussian {where[0]} word {where[1]}")
    assert k <= PR.KAPPA_REF, (k, where)


@pytest.mark.parametrize("name,t_min", CASES)
def test_bound_is_not_vacuous(oracle, name, t_min):
    r = PR.reference(name, t_min)
    g, b = PR.convert_rows(r["rows"], PR.row_bound(r, PR.KAPPA_TEST), r["pre"])
    mask = np.zeros(g.shape, bool); mask[PR.touched(r)] = True
    s3, s2 = PR.shares(g, b, mask)
    print(f"\nshares[{name}, t_min={t_min:g}]: bound <= 1e-3 |ref| {s3:.3f}, <= 1e-2 |ref| {s2:.3f}")
    assert name in PR.SPARSE + PR.DEEP and PR.bound_means_something(name, s3, s2), (s3, s2)


@pytest.mark.parametrize("name", SCENES_3D)
def test_sh_path_twin_stays_inside_kappa_sh_ref(oracle, name):
    """The backward's SH colour path: fp64 reference == the chain's colour part; the fp32 twin (the kernel's statements in float) stays
    inside KAPPA_SH_REF * 2^-24 * mass + floor on every output float; untouched gaussians stay exactly zero."""
    O = oracle
    s = PR.scene(name); sc = s["sc"]; r = PR.reference(name, 1e-5)
    n = s["n"]
    drgb32 = r["rows"][:, :3].astype(np.float32)                              # a colour gradient as a kernel holds it
    ref = O.sh_path(sc["means"], sc["shs"], s["deg"], s["ocam"], drgb32.astype(np.float64), omp=True)
    tw = O.sh_path_f32(sc["means"], sc["shs"], s["deg"], s["ocam"], drgb32, omp=True)
    rows = np.zeros((n, 10)); rows[:, :3] = drgb32
    g = O.chain(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], s["deg"], s["ocam"], rows, raw=True, omp=True)
    assert np.abs(g["shs"].reshape(n, -1) - ref["dshs"]).max() <= 1e-14 * np.abs(ref["dshs"]).max()
    sh = PR.sh_reference(name, dict(rows=rows))
    T = np.array(s["ocam"].T, np.float64).reshape(4, 4).T; P = np.array(s["ocam"].P, np.float64).reshape(4, 4).T
    dm = (ref["dpc"] @ P[:3, :] @ T)[:, :3]                                    # colour rows only: d means is T' P' [dpc; 0]
    assert np.abs(g["means"] - dm).max() <= 1e-12 * np.abs(dm).max()
    assert np.all(sh["A"] >= np.abs(P[:3, :] @ T[:, :3]))
    dead = ~np.any(drgb32 != 0, axis=1)
    worst = 0.0
    for k, mk in (("dshs", "mass_shs"), ("dpc", "mass_dpc")):
        assert np.all(tw[k][dead] == 0.0) and np.all(ref[k][dead] == 0.0) and np.isfinite(ref[mk]).all()
        e = np.maximum(np.abs(tw[k].astype(np.float64) - ref[k]) - PR.SH_FLOOR, 0.0); m = PR.U * ref[mk]
        assert np.all(e[m == 0] == 0.0)
        kap = float((e[m > 0] / m[m > 0]).max())
        print(f"\nkappa_sh_ref[{name}, {k}] = {kap:.3f}")
        worst = max(worst, kap)
    assert worst <= PR.KAPPA_SH_REF, worst


@pytest.mark.parametrize("name", ["deg2", "rawq"])
def test_parameter_level_bound_holds_for_the_twin(oracle, name):
    """Level 2 on the CPU: the twin's rows through the chain stay inside sum_i |J_oi| (row bound)_i around gso_chain(reference rows) --
    the Jacobians from unit rows and the bound's propagation, checked on rows whose error is known to be legitimate."""
    O = oracle
    s = PR.scene(name); sc = s["sc"]; r = PR.reference(name, 1e-5)
    tch = PR.touched(r)
    got = O.chain(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], s["deg"], s["ocam"], PR.twin(name, 1e-5).astype(np.float64), raw=True, omp=True)
    for k, (ref, b) in PR.chain_reference(name, r, PR.row_bound(r, PR.KAPPA_REF)).items():
        err = np.abs(got[k].reshape(ref.shape) - ref)
        assert np.all(err[tch] <= b[tch]), (k, float((err[tch] / np.maximum(b[tch], 1e-300)).max()))
        assert np.all(got[k].reshape(ref.shape)[~tch] == 0.0) and np.all(ref[~tch] == 0.0), k
        assert np.median(b[tch] / np.maximum(np.abs(ref[tch]), 1e-300)) <= 1e-3, k      # and means something


@pytest.mark.parametrize("t_min", [0.0, 1e-5])
def test_rows_of_the_2d_renderer_are_gso_backward2d(oracle, t_min):
    """The walk of gso_composite_rows is tied to composite_adjoint64's for the 2-D renderer too (tps == NULL: no near/far test): at the
    fp64 payload of gso_backward2d (Sigma = R S^2 R' + 0.3 I, mu = (W mx, H my), raw clamped opacity) the rows are its g2d."""
    O = oracle
    s = PR.scene("2d"); sc = s["sc"]; r = PR.reference("2d", t_min)
    W, H = s["W"], s["H"]
    gref = O.backward2d(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"], W, H, r["ranges"], r["ids"], s["dC"], t_min=t_min, omp=True)
    th = sc["rots"].astype(np.float64).reshape(-1); c, sn = np.cos(th), np.sin(th)
    e = np.exp(sc["scales"].astype(np.float64))
    Wm = np.stack([np.stack([c * e[:, 0], -sn * e[:, 1]], 1), np.stack([sn * e[:, 0], c * e[:, 1]], 1)], 1)          # [n, row, col]
    cov = Wm @ Wm.transpose(0, 2, 1) + 0.3 * np.eye(2)
    det = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    f = dict(M=np.stack([cov[:, 1, 1] / det, -cov[:, 1, 0] / det, -cov[:, 0, 1] / det, cov[:, 0, 0] / det], 1),
             mu=np.stack([float(W) * sc["means"][:, 0].astype(np.float64), float(H) * sc["means"][:, 1].astype(np.float64)], 1),
             sig=np.clip(sc["opacities"].reshape(-1), np.float32(0), np.float32(0.99999994)).astype(np.float64), rgb=sc["colors"].astype(np.float64))
    got = O.composite_rows(f, r["pre"]["bbs"], None, r["ranges"], r["ids"], s["ocam"], s["dC"], t_min=t_min, omp=True)
    ok = f["sig"] > 0
    f1 = dict(f, sig=np.where(ok, f["sig"], 1.0))
    conv = _convert64(got["rows"], f1)
    scale = np.abs(_convert64(got["mass"] / 8.0, dict(M=np.abs(f["M"]), sig=-f1["sig"])))
    assert ok.sum() > 0.99 * len(ok)
    assert np.all(np.abs(conv - gref["g2d"])[ok] <= (1e-12 * (np.abs(gref["g2d"]) + scale) + 1e-300)[ok]), np.abs(conv - gref["g2d"])[ok].max()


@pytest.mark.parametrize("name,t_min", CASES)
def test_converted_bound_holds_for_the_twin(oracle, name, t_min):
    """Level 1 on the CPU: the twin's rows through gs_g2d_to_grads<float> (restated in NumPy float32) stay inside the bound that
    convert_rows carries through that step, around the converted reference -- also with the allowances the modes add (they only widen it)."""
    r = PR.reference(name, t_min)
    tch = PR.touched(r)
    got = PR.g2d_to_grads_f32(PR.twin(name, t_min), r["pre"]).astype(np.float64)
    ref, b = PR.convert_rows(r["rows"], PR.row_bound(r, PR.KAPPA_REF), r["pre"])
    assert np.all(np.abs(got - ref)[tch] <= b[tch]), float((np.abs(got - ref)[tch] / np.maximum(b[tch], 1e-300)).max())
    assert np.all(got[~tch] == 0.0) and np.all(ref[~tch] == 0.0)
    wide = PR.row_bound(r, PR.KAPPA_REF, dropped=True, det_adds=8.0 * r["ntiles"])
    plain = PR.row_bound(r, PR.KAPPA_REF)
    assert np.all(wide >= plain) and np.all(wide[~tch] == 0.0)
    # the allowances are what they say: sum |term| below alpha 2^-27 is a sliver of the mass; 2^-41 (2^-29) per fixed-point add
    assert np.all(r["dropped"] <= r["mass"] / 8.0)
    extra = wide - plain - r["dropped"] - PR.U * np.abs(r["rows"])
    want = 8.0 * r["ntiles"][:, None] * np.where(np.arange(10) >= 6, 2.0 ** -29, 2.0 ** -41)[None, :]
    assert np.allclose(extra, want, rtol=1e-6, atol=1e-30)


def test_one_underflow_constant(oracle):
    assert PR.SH_FLOOR == oracle.floor_unit() == 2.0 ** -120
