"""Per-gaussian reference of the composite backward, shared by test_oracle_pergaussian.py (CPU) and test_gpu_pergaussian.py (GPU):
scenes, bounds and their propagation.

The reference is oracle.composite_rows: the fp64 composite adjoint AT THE fp32 PAYLOAD (which the GPU preprocess reproduces bit for
bit), with an error mass per (gaussian, component).  A correct fp32 evaluation of the adjoint stays inside

    kappa * 2^-24 * mass + floor (+ dropped, where entries below alpha = 2^-27 may be omitted whole)

KAPPA_REF is the largest kappa the fp32 twin (oracle.composite_rows_f32: the kernel's own formulation in float, on the CPU)
reaches over the scenes below; test_oracle_pergaussian.py re-measures it, prints it per scene and fails when it is exceeded.  The
GPU bar is KAPPA_TEST = 4 x KAPPA_REF: the factor covers what the twin does not mirror (the exp2 and reciprocal instructions in
place of expf and /, log2 e folded into the payload conic, fma formation, the order of the atomics) -- each a constant number of ulps on
quantities the mass already weighs.  KAPPA_TEST is never fitted to what a kernel gives.
"""
import numpy as np

U = 2.0 ** -24
KAPPA_REF = 0.8            # the largest the twin reaches is 0.756 (scene deg1); per scene: profiles/pergaussian_bounds.log
KAPPA_TEST = 4.0 * KAPPA_REF

# (name, kind, n, W, H, sh degree, seed): the smallest scenes that still have the structure -- ragged sizes, several SH degrees, a dense
# scene whose lists run to several hundred entries (pixels freeze), raw quaternions, the 2-D renderer
SCENES = {
    "deg1": ("3d", 3001, 200, 120, 1, 7),
    "deg3": ("3d", 4097, 176, 90, 3, 9),
    "deg2": ("3d", 2500, 136, 104, 2, 8),
    "dense": ("dense", 4000, 80, 56, 2, 17),
    "rawq": ("rawq", 2049, 200, 120, 1, 21),
    "2d": ("2d", 1501, 200, 120, 0, 6),
    # heavy-tailed, on a grid with a launch order (3072 tiles: more than half the wave slots): the smallest at which tile_lpt_order_kernel splits tiles
    "clustered": ("clustered", 150_000, 1024, 768, 1, 1236),
}
# Non-vacuity (a case fails outside these): in a sparse scene at least 90 % of the touched (gaussian, component) pairs have a bound within
# 1e-3 of |reference|; in a deep one (lists of several batches: gaussians far behind a saturated pixel have gradients at the level of the
# cancellation in S, which the bound must allow) at least 75 % within 1e-2.  Unnormalised quaternions inflate every footprint by |q|^4
# (|q|^2 ~ chi^2_4: a heavy tail), so that scene is deep even with its scales lowered by 2.5.
SPARSE = ("deg1", "deg3", "deg2", "2d")
DEEP = ("dense", "rawq")
# The heavy-tailed scene (GPU only: it is large) is there for the tiles the launch order splits.  Most of its gaussians are faint members
# of blobs whose tiles walk thousands of entries far behind saturated pixels; the non-vacuity conditions are stated for the sparse and the
# dense scenes, so its shares are printed and carry no bar of their own.
HEAVY = ("clustered",)


def bound_means_something(name, s3, s2):
    return s3 >= 0.90 if name in SPARSE else (s2 >= 0.75 if name in DEEP else True)


ROW_USED = [0, 1, 2, 3, 4, 5, 6, 7, 9]      # words of a device row that carry a sum (8 is padding)

_cache = {}


def scene(name):
    """-> dict(kind, sc, W, H, deg, seed, dC, and for 3-D scenes cam, T, P, ocam); built once, never modified"""
    if name in _cache:
        return _cache[name]
    from gaussiansplat_amd import camera as gcam, synthetic
    from oracle import oracle as O
    kind, n, W, H, deg, seed = SCENES[name]
    s = dict(kind=kind, n=n, W=W, H=H, deg=deg, seed=seed, dC=synthetic.make_dC(W, H, seed))
    if kind == "2d":
        s["sc"] = synthetic.make_scene_2d(n, W, H, seed, scale_hi=1.0)     # log-scales U[0,1): the reference's own draw (splat.jl:74-87)
        s["ocam"] = O.image_camera(W, H)
    else:
        sc = synthetic.make_scene(n, W, H, deg, seed=seed, raw_quaternions=(kind == "rawq"), clustered=(kind == "clustered"))
        if kind == "dense":
            sc["scales"] = (sc["scales"] + np.float32(1.2)).astype(np.float32)
        if kind == "rawq":
            sc["scales"] = (sc["scales"] - np.float32(2.5)).astype(np.float32)
        cam = synthetic.scene_camera(W, view=0)
        T = gcam.compute_transform(cam); P = gcam.compute_projection(cam, W, H)
        s.update(sc=sc, cam=cam, T=T, P=P,
                 ocam=O.camera_from_arrays(T, P, np.float32(cam.fx), np.float32(cam.fy), np.float32(cam.near), np.float32(cam.far),
                                           cam.eye, cam.lookAt, W, H))
    _cache[name] = s
    return s


def reference(name, t_min, order=1):
    """The oracle's frame of a scene and the per-gaussian reference of its composite backward; cached per (scene, t_min, order)."""
    s = scene(name); sc = s["sc"]
    if s["kind"] == "2d":
        order = 0                                           # the 2-D renderer has no depth: lists in gaussian-index order
    key = (name, float(t_min), order)
    if key in _cache:
        return _cache[key]
    from oracle import oracle as O
    if s["kind"] == "2d":
        ref = O.render2d(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"], s["W"], s["H"], t_min=t_min, omp=True)
        tps = None
    else:
        ref = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], s["deg"], s["ocam"], order=order, t_min=t_min, omp=True)
        tps = ref["pre"]["tps"]
    pre = ref["pre"]
    r = O.composite_rows(pre, pre["bbs"], tps, ref["ranges"], ref["ids"], s["ocam"], s["dC"], t_min=t_min, omp=True)
    r.update(pre=pre, ranges=ref["ranges"], ids=ref["ids"], image=ref["image"], trans=ref["trans"], tps=tps)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = r
    return r


def twin(name, t_min, order=1):
    from oracle import oracle as O
    s = scene(name); r = reference(name, t_min, order)
    return O.composite_rows_f32(r["pre"], r["ranges"], r["ids"], s["ocam"], s["dC"], t_min=t_min, use_tps=r["tps"] is not None, omp=True)


def row_bound(r, kappa, dropped=False, det_adds=None):
    """Bound [n,10] on |fp32 row - r['rows']|.  dropped: entries below alpha 2^-27 may be missing.  det_adds [n]: number of fixed-point
    adds a gaussian's sums may have taken (deterministic mode): each rounds to 2^-40 (2^-28 for the second moments), i.e. errs by half."""
    b = kappa * U * r["mass"] + r["floor"]
    if dropped:
        b = b + r["dropped"]
    if det_adds is not None:
        res = np.full(10, 2.0 ** -41); res[6:] = 2.0 ** -29
        b = b + np.asarray(det_adds, np.float64)[:, None] * res[None, :]
        b = b + U * np.abs(r["rows"])                      # the read-back rounds the fixed-point sum to float
    return b


def kappa_of(got_rows, r, extra=0.0):
    """Largest (|got - ref| - floor - extra) / (2^-24 mass) over the touched (gaussian, component) pairs, and where."""
    err = np.abs(np.asarray(got_rows, np.float64) - r["rows"]) - r["floor"] - extra
    m = r["mass"][:, ROW_USED]
    e = err[:, ROW_USED]
    ratio = np.where(m > 0, np.maximum(e, 0.0) / np.where(m > 0, U * m, 1.0), np.where(e > 0, np.inf, 0.0))
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), (int(i[0]), ROW_USED[i[1]])


def convert_rows(rows, bound, pre):
    """The read-back's raw -> d{sig, mu, conic} step (gs_g2d_to_grads<float> with the fp32 sig and conic), in float64 on the reference
    rows, and the bound carried through it: the step is linear with known coefficients; its own fp32 operations add a few ulps of
    the absolute-valued terms.  -> (grads [n,10], bound [n,10]) in ARR_GRAD2D's layout [dr dg db dsig dmx dmy d00 d01 d10 d11]."""
    sig = np.asarray(pre["sig"], np.float64).reshape(-1)
    ic = np.asarray(pre["invcov"], np.float32)
    i0 = ic[:, 0].astype(np.float64); i3 = ic[:, 3].astype(np.float64)
    mc = (np.float32(0.5) * (ic[:, 1] + ic[:, 2])).astype(np.float64)
    S0, Sx, Sy, Sxx, Sxy, Syy = (rows[:, c] for c in (3, 4, 5, 6, 7, 9))
    b0, bx, by, bxx, bxy, byy = (bound[:, c] for c in (3, 4, 5, 6, 7, 9))
    g = np.zeros_like(rows); b = np.zeros_like(rows)
    g[:, :3] = rows[:, :3]; b[:, :3] = bound[:, :3]
    ok = sig > 0
    sg = np.where(ok, sig, 1.0)
    g[:, 3] = np.where(ok, -S0 / sg, 0.0); b[:, 3] = np.where(ok, b0 / sg + U * np.abs(S0 / sg), 0.0)
    ax = np.abs(i0 * Sx) + np.abs(mc * Sy); ay = np.abs(mc * Sx) + np.abs(i3 * Sy)
    g[:, 4] = -(i0 * Sx + mc * Sy); b[:, 4] = np.abs(i0) * bx + np.abs(mc) * by + 3 * U * ax
    g[:, 5] = -(mc * Sx + i3 * Sy); b[:, 5] = np.abs(mc) * bx + np.abs(i3) * by + 3 * U * ay
    g[:, 6] = 0.5 * Sxx; b[:, 6] = 0.5 * bxx
    g[:, 7] = g[:, 8] = 0.5 * Sxy; b[:, 7] = b[:, 8] = 0.5 * bxy
    g[:, 9] = 0.5 * Syy; b[:, 9] = 0.5 * byy
    return g, b


def g2d_to_grads_f32(rows32, pre):
    """gs_g2d_to_grads<float> restated in NumPy float32, operation by operation: what the read-back applies to a device row"""
    r = np.asarray(rows32, np.float32)
    sig = np.asarray(pre["sig"], np.float32).reshape(-1); ic = np.asarray(pre["invcov"], np.float32)
    i0, i3 = ic[:, 0], ic[:, 3]
    mc = np.float32(0.5) * (ic[:, 1] + ic[:, 2])
    S0, Sx, Sy, Sxx, Sxy, Syy = (r[:, c] for c in (3, 4, 5, 6, 7, 9))
    g = np.zeros_like(r)
    g[:, :3] = r[:, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        g[:, 3] = np.where(sig > 0, -S0 / sig, np.float32(0))
    g[:, 4] = -(i0 * Sx + mc * Sy)
    g[:, 5] = -(mc * Sx + i3 * Sy)
    g[:, 6] = np.float32(0.5) * Sxx; g[:, 7] = g[:, 8] = np.float32(0.5) * Sxy; g[:, 9] = np.float32(0.5) * Syy
    return g


def touched(r):
    return r["ntiles"] > 0


def shares(ref_vals, bound, mask):
    """Non-vacuity: shares of the touched (gaussian, component) pairs whose bound is within 1e-3 and 1e-2 of |reference|."""
    v = np.abs(ref_vals[mask]); b = bound[mask]
    return float(np.mean(b <= 1e-3 * v)), float(np.mean(b <= 1e-2 * v))


# ---------------------------------------------------------------- level 2: the parameter chain

GEOM = ("means", "scales", "quats", "opacities", "shs")
# The SH colour path (direction, basis, d_shs, the colour's pull on the position) is the part of the chain the kernels run in fp32:
# oracle.sh_path states its error mass, oracle.sh_path_f32 (the kernel's statements in float) measures what a correct evaluation
# uses -- at most 0.27 over the scenes (test_oracle_pergaussian.py prints it); the GPU bar is 4 x the pinned value, as for the composite
# (the twin has 1 / sqrtf where the kernel has the reciprocal square root instruction).  SH_FLOOR: a product that underflows loses at most
# 2^-126 before the remaining factors (|basis| < 4, 1 / |v| < 2^4) multiply it: oracle.floor_unit(), the constant the composite floor uses.
KAPPA_SH_REF = 0.3
KAPPA_SH_TEST = 4.0 * KAPPA_SH_REF
SH_FLOOR = 2.0 ** -120       # == oracle.floor_unit() (test_oracle_pergaussian.py asserts it)


def jacobians(name):
    """d(parameter gradient) / d(device row word) per gaussian, from oracle.chain on unit rows (the chain is linear in the row and
    every gaussian's is independent): {param: [n, width, 10]}.  Cached per scene."""
    key = (name, "jac")
    if key in _cache:
        return _cache[key]
    from oracle import oracle as O
    s = scene(name); sc = s["sc"]; n = s["n"]
    K3 = 3 * (s["deg"] + 1) ** 2
    J = {k: np.zeros((n, w, 10)) for k, w in (("means", 3), ("scales", 3), ("quats", 4), ("opacities", 1), ("shs", K3))}
    for c in ROW_USED:
        rows = np.zeros((n, 10)); rows[:, c] = 1.0
        g = O.chain(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], s["deg"], s["ocam"], rows, raw=True, omp=True)
        for k in J:
            J[k][:, :, c] = g[k].reshape(n, -1)
    _cache[key] = J
    return J


def sh_reference(name, r):
    """oracle.sh_path at the reference's colour gradient, and |d means / d dpc| (means = T' P' [dpc; 0], absolute-valued)"""
    from oracle import oracle as O
    s = scene(name); sc = s["sc"]
    sh = O.sh_path(sc["means"], sc["shs"], s["deg"], s["ocam"], r["rows"][:, :3], omp=True)
    T = np.array(s["ocam"].T, np.float64).reshape(4, 4).T; P = np.array(s["ocam"].P, np.float64).reshape(4, 4).T     # [row, col]
    sh["A"] = (np.abs(P[:3, :]) @ np.abs(T[:, :3]))                                                                     # [dpc a, mean j]
    return sh


def chain_reference(name, r, rbound):
    """Parameter-level reference gso_chain(reference rows) and its bound per output float: sum_i |J_oi| (row bound)_i, plus
    2 * 2^-24 |ref| for the fp32 store, plus 1e-12 of the absolute-valued chain for the two fp64 evaluations' own rounding, plus -- d_shs and
    d_means -- the SH path's mass at KAPPA_SH_TEST."""
    from oracle import oracle as O
    s = scene(name); sc = s["sc"]; n = s["n"]
    g = O.chain(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], s["deg"], s["ocam"], r["rows"], raw=True, omp=True)
    J = jacobians(name)
    sh = sh_reference(name, r)
    extra = dict(shs=KAPPA_SH_TEST * U * sh["mass_shs"] + SH_FLOOR,
                 means=(KAPPA_SH_TEST * U * sh["mass_dpc"] + SH_FLOOR) @ sh["A"])
    out = {}
    for k in GEOM:
        ref = g[k].reshape(n, -1)
        aJ = np.abs(J[k])
        b = np.einsum("noc,nc->no", aJ, rbound) + 2 * U * np.abs(ref) + 1e-12 * np.einsum("noc,nc->no", aJ, np.abs(r["rows"]))
        if k in extra:
            b = b + np.where((r["ntiles"] > 0)[:, None], extra[k], 0.0)
        out[k] = (ref, b)
    return out
