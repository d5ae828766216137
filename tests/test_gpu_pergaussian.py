"""Per-gaussian gradient parity of the HIP backward with rounding-aware bounds (run on the MI355X: pytest -m gpu).

The other parity tests hold a whole gradient array to one rel-L2 number, which an error confined to a few gaussians -- the last entry
before a segment boundary, the entries a second pixel part owns, a tile that extends a capped list, a snapshot restored one entry
off -- passes.  Here EVERY gaussian and EVERY component is held to a bound of its own, against a reference that takes the fp32
payload as given (tests/pergaussian_ref.py, oracle/gs_oracle.c: gso_composite_rows):

  level 0  a gaussian no pixel takes (mass == 0) has all-zero gradient rows, every float; nothing anywhere is non-finite;
  level 1  ARR_GRAD2D against the reference's raw moments put through the read-back's own conversion, inside
           KAPPA_TEST * 2^-24 * mass + floor (+ dropped where entries below alpha 2^-27 may be omitted: alpha_cull, several waves
           per tile; + the fixed-point allowance in deterministic mode), the bound carried through the conversion;
  level 2  the parameter gradients against gso_chain(reference rows), inside sum_i |J_oi| (row bound)_i + 2 * 2^-24 |ref|, plus
           the mass of the SH colour path (fp32 in the kernels) for d_shs and d_means.

KAPPA_TEST = 4 x the kappa a correct fp32 evaluation reaches on the CPU (test_oracle_pergaussian.py); it is not fitted to the kernels.
Every case on a sparse or dense scene also fails if its bound stops meaning something (pergaussian_ref.SPARSE / DEEP shares) and asserts that the mode it
names engaged, the way the mode's own tests do.  The figures each case reaches are printed (profiles/pergaussian_bounds.log).
"""
import numpy as np
import pytest

import pergaussian_ref as PR
from common import hip_context, run_frame

pytestmark = pytest.mark.gpu

SEG_MAX = 8                 # GS_SEG_MAX: list segments a tile's backward may run as


def _ctx(s, **kw):
    from gaussiansplat_amd import backend as B
    sc = s["sc"]
    if s["kind"] == "2d":
        ctx = B.Context(order=B.ORDER_INDEX, **kw)
        ctx.set_model_2d_host(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"])
        ctx.set_image_size(s["W"], s["H"])
        return ctx
    return hip_context(sc, s["cam"], s["T"], s["P"], s["W"], s["H"], s["deg"], order=1, **kw)


def _frame(ctx, s, **kw):
    return run_frame(ctx, s["dC"], s["deg"], kind=s["kind"], g2d=True, **kw)


def _worst(err, bound, sel):
    """largest err / bound over the selected floats (0/0 = 0), and its index"""
    q = np.where(sel, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), 0.0)
    i = np.unravel_index(np.argmax(q), q.shape)
    return float(q[i]), tuple(int(v) for v in i)


def _check(name, t_min, f, label, det, may_drop):
    """levels 0, 1, 2 of one frame; every level is evaluated before anything is asserted, so a failure names all that broke"""
    s = PR.scene(name); r = PR.reference(name, t_min)
    tch = PR.touched(r)
    g2d = f["g2d"].astype(np.float64)
    fails = []
    # ---- level 0
    if not np.isfinite(g2d).all() or not all(np.isfinite(v).all() for v in f["grads"].values()):
        fails.append("level 0: non-finite gradient")
    if np.any(f["g2d"][~tch] != 0.0):
        fails.append(f"level 0: ARR_GRAD2D rows of untouched gaussians {np.nonzero(np.any(f['g2d'][~tch] != 0.0, axis=1))[0][:5]}")
    for k, v in f["grads"].items():
        if np.any(v.reshape(len(tch), -1)[~tch] != 0.0):
            fails.append(f"level 0: d_{k} of untouched gaussians")
    # ---- level 1
    adds = r["ntiles"].astype(np.float64) * f["parts"] * SEG_MAX if det else None
    b0 = PR.convert_rows(r["rows"], PR.row_bound(r, 0.0, dropped=may_drop, det_adds=adds), r["pre"])[1]
    rb = PR.row_bound(r, PR.KAPPA_TEST, dropped=may_drop, det_adds=adds)
    ref, b = PR.convert_rows(r["rows"], rb, r["pre"])
    err = np.abs(g2d - ref)
    sel = np.zeros(ref.shape, bool); sel[tch] = True
    w1, at1 = _worst(err, b, sel)
    per_kappa = (b - b0) / PR.KAPPA_TEST                                   # what one unit of kappa buys, through the conversion
    kap, _ = _worst(np.maximum(err - b0, 0.0), per_kappa, sel)
    # non-vacuity is a property of the mass: shares at the plain bound kappa * 2^-24 * mass + floor (the mode's allowances -- dropped, the
    # fixed-point adds, stated as upper limits -- come on top of it in the comparison above)
    s3, s2 = PR.shares(ref, PR.convert_rows(r["rows"], PR.row_bound(r, PR.KAPPA_TEST), r["pre"])[1], sel)
    if w1 > 1.0:
        fails.append(f"level 1: gaussian {at1[0]} word {at1[1]}: |got - ref| = {err[at1]:.3e} is {w1:.2f} x its bound {b[at1]:.3e} (ref {ref[at1]:.3e})")
    if not PR.bound_means_something(name, s3, s2):
        fails.append(f"vacuous bound: shares {s3:.3f} / {s2:.3f}")
    # ---- level 2
    w2, line2 = 0.0, ""
    if s["kind"] != "2d":
        for k, (pref, pb) in PR.chain_reference(name, r, rb).items():
            got = f["grads"][k].astype(np.float64).reshape(pref.shape)
            perr = np.abs(got - pref)
            psel = np.zeros(pref.shape, bool); psel[tch] = True
            w, at = _worst(perr, pb, psel)
            line2 += f" {k} {w:.3f}"
            w2 = max(w2, w)
            if w > 1.0:
                fails.append(f"level 2: d_{k}[{at[0]}, {at[1]}]: |got - ref| = {perr[at]:.3e} is {w:.2f} x its bound {pb[at]:.3e} (ref {pref[at]:.3e})")
    print(f"\npergaussian[{name} t_min={t_min:g} {label}]: touched {int(tch.sum())}, level 1 kappa reached {kap:.3f} of {PR.KAPPA_TEST:g}, "
          f"err/bound {w1:.3f}; level 2 err/bound{line2 or ' -'}; shares {s3:.3f} / {s2:.3f}")
    assert not fails, "\n".join(fails)


BASE = [(name, t, det, cull) for name in PR.SCENES if name != "clustered"
        for (t, det, cull) in ((0.0, False, True), (1e-5, False, True), (1e-5, True, True), (1e-5, False, False), (0.0, True, False))]
BASE += [("dense", 0.2, False, True), ("dense", 0.2, True, False), ("dense", 0.2, True, True)]


@pytest.mark.parametrize("name,t_min,det,cull", BASE)
def test_one_wave_per_tile(oracle, name, t_min, det, cull):
    """t_min 0 / 1e-5 / 0.2, float and fixed-point atomics, the no-op cull on and off: whole tiles, full lists, accumulate"""
    s = PR.scene(name)
    ctx = _ctx(s, t_min=t_min, deterministic=det, alpha_cull=cull, tile_parts=1, slab_mode=0, list_cap=1)
    f = _frame(ctx, s)
    ctx.close()
    assert f["parts"] == 1 and f["rounds"] == 1 and not f["st"]["capped"]
    assert f["wc"]["walked_fwd"] == f["wc"]["walked_bwd"] > 0
    assert f["wc"]["evaluated_fwd"] == f["wc"]["evaluated_bwd"]
    assert (f["wc"]["evaluated_bwd"] <= f["wc"]["walked_bwd"]) if cull else (f["wc"]["evaluated_bwd"] == f["wc"]["walked_bwd"])
    _check(name, t_min, f, f"det={int(det)} cull={int(cull)}", det, may_drop=cull)


@pytest.mark.parametrize("name", ["deg1", "dense"])
@pytest.mark.parametrize("parts", [2, 4])
@pytest.mark.parametrize("det", [False, True])
def test_pixel_parts(oracle, name, parts, det):
    """two and four waves per tile, each differentiating its own strips (the entries a second pixel part owns)"""
    s = PR.scene(name)
    ctx = _ctx(s, t_min=1e-5, deterministic=det, tile_parts=parts, slab_mode=0, list_cap=1)
    f = _frame(ctx, s)
    ctx.close()
    assert f["parts"] == parts
    _check(name, 1e-5, f, f"tile_parts={parts} det={int(det)}", det, may_drop=True)


@pytest.mark.parametrize("name", ["deg3", "dense"])
@pytest.mark.parametrize("det", [False, True])
def test_view_slot_list_segments(oracle, name, det):
    """tile_parts = 0 under a view slot: the first frame runs pixel parts, the next ones every tile's backward as two segments of its
    list from the forward's snapshots, two entries in flight (PAIR) -- each of the three frames is held to the bound"""
    s = PR.scene(name)
    ctx = _ctx(s, t_min=1e-5, deterministic=det, tile_parts=0)
    first = None
    for frame in (1, 2, 3):
        f = _frame(ctx, s, slot=2)
        first = first or f
        assert f["wc"]["walked_bwd"] >= first["wc"]["walked_bwd"] > 0         # (the segments' sum is the tile's whole walk)
        _check(name, 1e-5, f, f"view slot frame {frame} det={int(det)}", det, may_drop=True)
    ctx.close()


def test_heavy_tiles_split_by_the_launch_order(oracle):
    """GS_DEBUG_ALWAYS_ORDER on the heavy-tailed scene, frames under one view slot: from the second frame on the forward runs on the slot's
    launch order, whose heaviest tiles are split into pixel parts; their backward runs as segments of their lists from the forward's snapshots"""
    from gaussiansplat_amd import backend as B
    s = PR.scene("clustered")
    ctx = _ctx(s, t_min=1e-5, tile_parts=0, debug_flags=B.GS_DEBUG_ALWAYS_ORDER)
    for frame in (1, 2, 3):
        f = _frame(ctx, s, slot=0)
    front = 2304                                                               # GS_LPT_FRONT: the order's entries for the extra waves of split tiles
    units = int((ctx.tile_clock(0, -30)[:front, 1] > 0).sum())                 # (a debug forward launch over the last frame's order)
    ctx.close()
    assert units >= 8, units                                                   # the blobs' tiles are split
    _check("clustered", 1e-5, f, f"launch order, {units} split units, frame 3", False, may_drop=True)


@pytest.mark.parametrize("det", [False, True])
def test_tiny_caps_extend_lists_in_the_kernel(oracle, det):
    """list_cap = 2 with GS_DEBUG_TINY_CAPS: every busy tile's list is written short and extended by the forward's waves; the backward
    stops where the forward stopped (a tile that extends a capped list)"""
    from gaussiansplat_amd import backend as B
    s = PR.scene("dense")
    ctx = _ctx(s, t_min=1e-5, deterministic=det, list_cap=2, slab_mode=0, tile_parts=1, debug_flags=B.GS_DEBUG_TINY_CAPS)
    for frame in (1, 2):
        f = _frame(ctx, s)
        assert f["st"]["capped"] and f["st"]["listed"] <= ctx.num_instances
        _check("dense", 1e-5, f, f"tiny caps frame {frame} det={int(det)}", det, may_drop=True)
    ctx.close()


@pytest.mark.parametrize("fractions,rounds", [((0.3,), 2), ((0.1, 0.2, 0.4), 4)])
@pytest.mark.parametrize("det", [False, True])
def test_forced_slabs(oracle, fractions, rounds, det):
    """frames binned in depth slabs: the backward walks a tile's list as the concatenation of the rounds' segments"""
    s = PR.scene("dense")
    ctx = _ctx(s, t_min=1e-5, deterministic=det, slab_mode=1, slab_fractions=fractions, tile_parts=1)
    f = _frame(ctx, s)
    ctx.close()
    assert f["rounds"] == rounds and f["wc"]["walked_bwd"] == f["wc"]["walked_fwd"] > 0
    _check("dense", 1e-5, f, f"slabs {fractions} det={int(det)}", det, may_drop=True)


@pytest.mark.parametrize("name", ["deg2", "rawq"])
@pytest.mark.parametrize("no_fill", [False, True])
def test_overwrite_with_and_without_tail_fill(oracle, name, no_fill):
    """an overwriting backward (against the accumulating one of the other cases), its zero fills carried in the ragged end of the composite
    launches or (GS_DEBUG_NO_TAIL_FILL) in line; the second frame's forward carries the fill of the 2-D rows"""
    from gaussiansplat_amd import backend as B
    s = PR.scene(name)
    ctx = _ctx(s, t_min=1e-5, deterministic=True, bin_path=3, tile_parts=1, debug_flags=B.GS_DEBUG_NO_TAIL_FILL if no_fill else 0)
    for frame in (1, 2):
        f = _frame(ctx, s, overwrite=True)
        fill = ctx.tail_fill_blocks()
        assert (fill == (0, 0)) if no_fill else (fill[1] > 0), fill
        _check(name, 1e-5, f, f"overwrite no_fill={int(no_fill)} frame {frame}", True, may_drop=True)
    ctx.close()


@pytest.mark.parametrize("name", ["deg3", "2d"])
def test_composite_then_params(oracle, name):
    """GS_BWD_COMPOSITE_ONLY followed by GS_BWD_PARAMS_ONLY (a multi-GPU host runs the phases apart)"""
    s = PR.scene(name)
    ctx = _ctx(s, t_min=1e-5, tile_parts=1)
    f = _frame(ctx, s, phases=("composite", "params"))
    ctx.close()
    _check(name, 1e-5, f, "composite only, then params only", False, may_drop=True)
