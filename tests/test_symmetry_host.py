"""The row symmetries on the CPU: the oracle holds them on exactly the inputs the GPU tests use, and the helpers of tests/symmetry.py have teeth.

The oracle's covariance is the evidence that the property tests/test_gpu_symmetry.py asks of the HIP path is real for a correct implementation:
with distinct depth keys, permuting the model's rows leaves image, transmittance, tile ranges and sorted keys as they are and permutes the
ids; inserting dead rows (a mean far off screen, a NaN mean) leaves them as they are on the live rows; and the fp64 adjoint's gradient rows
travel with their gaussians, bit for bit, with all-zero rows for gaussians off screen.  The teeth: distinct_key_scene really removes ties,
same_frame fails on one ulp in one float of one row and on a row map that is off by one, and padded keeps the live rows in order."""
import numpy as np
import pytest

import symmetry as S
from common import GRADS, same_bits, scene_and_cameras

SCENES = [(3000, 160, 96, 1, 41, 2.0), (2999, 200, 120, 3, 7, 0.0), (1000, 80, 56, 2, 17, 1.2)]   # n, W, H, degree, seed, scale boost
T_MIN = 1e-5
ROW_COUNTS = (1, 3072, 4097)                                                 # n + 1, and the two totals (where they exceed n)


def _args(sc):
    return sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"]


def _render(O, sc, deg, ocam, order):
    return O.render(*_args(sc), deg, ocam, order=order, t_min=T_MIN)


def _same_lists(base, other, to_base):
    """image, transmittance, ranges, keys equal; other's ids name base's gaussians through to_base"""
    for k in ("image", "trans", "ranges", "keys"):
        assert same_bits(base[k], other[k]), k
    assert same_bits(base["ids"], to_base[other["ids"]].astype(np.uint32)), "ids"


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("case", SCENES, ids=lambda c: "n%d" % c[0])
def test_oracle_is_covariant_under_permutation_and_padding(oracle, case, order):
    O = oracle
    n, W, H, deg, seed, boost = case
    sc, cam, T, P, ocam = S.distinct_key_scene(n, W, H, deg, seed, boost)
    rng = np.random.default_rng(seed)
    base = _render(O, sc, deg, ocam, order)
    assert len(base["ids"]) > n                                              # (a frame with real lists)
    # ---- permutation
    perm = rng.permutation(n)
    _same_lists(base, _render(O, S.permuted(sc, perm), deg, ocam, order), perm)
    # ---- padding
    for total in ROW_COUNTS:
        total = n + 1 if total == 1 else total
        if total <= n:
            continue
        pad, live, dead = S.padded(sc, total, rng)
        assert len(dead["offscreen"]) + len(dead["nan"]) == total - n and (total - n < 2 or min(len(v) for v in dead.values()) > 0)
        to_base = np.full(total, -1, np.int64); to_base[live] = np.arange(n)
        got = _render(O, pad, deg, ocam, order)
        assert not np.isin(np.concatenate(list(dead.values())), got["ids"]).any()       # dead rows reach no list
        _same_lists(base, got, to_base)


@pytest.mark.parametrize("case", SCENES, ids=lambda c: "n%d" % c[0])
def test_oracle_adjoint_rows_travel_with_their_gaussians(oracle, case):
    from gaussiansplat_amd import synthetic
    O = oracle
    n, W, H, deg, seed, boost = case
    sc, cam, T, P, ocam = S.distinct_key_scene(n, W, H, deg, seed, boost)
    rng = np.random.default_rng(seed + 1)
    dC = synthetic.make_dC(W, H, seed)

    def adjoint(s):
        r = _render(O, s, deg, ocam, 1)
        return O.backward(*_args(s), deg, ocam, r["ranges"], r["ids"], dC, t_min=T_MIN)
    base = adjoint(sc)
    assert all(np.any(base[k] != 0.0) for k in GRADS)
    perm = rng.permutation(n)
    got = S.unpermuted(adjoint(S.permuted(sc, perm)), perm)
    for k in base:
        assert S.first_difference(base[k], got[k]) is None, (k, S.first_difference(base[k], got[k]))
    pad, live, dead = S.padded(sc, 3072, rng)
    got = adjoint(pad)
    for k in base:
        assert S.first_difference(base[k], got[k][live]) is None, (k, S.first_difference(base[k], got[k][live]))
        assert S.rows_all_zero(got[k], dead["offscreen"]), k


def test_oracle_2d_is_invariant_under_padding(oracle):
    """the 2-D renderer (index order): rows outside the image are dead whatever t_min is; transparent rows are listed, so they are dead only
    without the early-out, whose batch boundaries are list positions (Early-out)"""
    from gaussiansplat_amd import synthetic
    O = oracle
    n, W, H = 900, 100, 60
    sc = synthetic.make_scene_2d(n, W, H)
    args = lambda s: (s["means"], s["scales"], s["rots"], s["opacities"], s["colors"], W, H)
    for t_min, kinds in ((0.0, ("outside",)), (T_MIN, ("outside",)), (0.0, S.KINDS_2D)):
        base = O.render2d(*args(sc), t_min=t_min)
        for total in (n + 1, 3072, 4097):
            pad, live, dead = S.padded(sc, total, np.random.default_rng(total), kinds)
            got = O.render2d(*args(pad), t_min=t_min)
            assert same_bits(base["image"], got["image"]) and same_bits(base["trans"], got["trans"]), (t_min, kinds, total)
            if kinds == ("outside",):
                to_base = np.full(total, -1, np.int64); to_base[live] = np.arange(n)
                assert same_bits(base["ranges"], got["ranges"]) and same_bits(base["ids"], to_base[got["ids"]].astype(np.uint32))


# ---------------------------------------------------------------- teeth
def test_distinct_key_scene_removes_forced_ties(oracle):
    n, W, H, deg = 400, 80, 56, 1
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 5)
    sc = {k: np.array(v, np.float32) for k, v in sc.items()}
    sc["means"][10:20, 2] = sc["means"][10, 2]                               # ten gaussians at one depth ...
    sc["means"][10:20, :2] = sc["means"][10, :2]                             # ... and on one ray: one key
    sc["means"][300] = sc["means"][30]                                       # and an exact duplicate
    for order in (1, 2):
        keys = S.depth_keys(sc, deg, ocam, order)
        assert np.unique(keys).size <= n - 10
    before = sc["means"].copy()
    nudges = S.remove_ties(sc, deg, ocam)
    assert nudges >= 10
    for order in (1, 2):
        keys = S.depth_keys(sc, deg, ocam, order)
        assert np.unique(keys).size == n
    assert np.array_equal(sc["means"][:, :2], before[:, :2])
    assert np.all(np.abs(sc["means"][:, 2] - before[:, 2]) <= 64 * 2.0 ** -23 * np.abs(before[:, 2]) + 1e-30)            # nudges of a few ulp, not moves
    assert same_bits(sc["means"][10], before[10]) and same_bits(sc["means"][30], before[30])                              # the first of each tie stays
    # which gaussian of a pair moves is decided by content: the tied scene, permuted, comes out as the permuted result
    tied = {k: v.copy() for k, v in sc.items()}; tied["means"] = before.copy()
    tied["means"][40:45, 2] = tied["means"][40, 2]; tied["means"][40:45, 1] = tied["means"][40, 1]              # one depth, x apart
    tied["means"][40:45, 0] = tied["means"][40, 0] + np.float32([0.0, -0.3, 0.2, -0.1, 0.4]) * np.float32(1e-3)
    perm = np.random.default_rng(2).permutation(n)
    keep = (perm != 10) & (perm != 30) & (perm != 300) & ~((perm >= 11) & (perm < 20))      # (identical gaussians can only go by their rows)
    a, b = {k: v.copy() for k, v in tied.items()}, S.permuted(tied, perm)
    assert S.remove_ties(a, deg, ocam) >= 14 and S.remove_ties(b, deg, ocam) >= 14
    assert same_bits(S.permuted(a["means"], perm)[keep], b["means"][keep])
    only = np.zeros(n, bool); only[:10] = True                                               # rows: ties outside the mask stay
    c = {k: v.copy() for k, v in tied.items()}
    assert S.remove_ties(c, deg, ocam, rows=only) == 0 and same_bits(c["means"], tied["means"])
    # the three scenes of the tests: asserted inside
    for n, W, H, deg, seed, boost in SCENES:
        S.distinct_key_scene(n, W, H, deg, seed, boost)


def _frame(rng, n, g2d=True):
    f = dict(img=rng.standard_normal((3, 8, 8)).astype(np.float32), tr=rng.random((8, 8)).astype(np.float32),
             grads=dict(means=rng.standard_normal((n, 3)).astype(np.float32), scales=rng.standard_normal((n, 3)).astype(np.float32),
                        quats=rng.standard_normal((n, 4)).astype(np.float32), opacities=rng.standard_normal(n).astype(np.float32),
                        shs=rng.standard_normal((n, 12)).astype(np.float32)))
    if g2d:
        f["g2d"] = rng.standard_normal((n, 10)).astype(np.float32)
    return f


def _copy(f):
    out = {k: (v.copy() if k != "grads" else {g: a.copy() for g, a in v.items()}) for k, v in f.items()}
    return out


def _moved(f, fn):
    """the frame with fn applied to every per-gaussian array"""
    out = _copy(f)
    out["grads"] = {k: fn(v) for k, v in f["grads"].items()}
    if "g2d" in f:
        out["g2d"] = fn(f["g2d"])
    return out


def test_same_frame_has_teeth():
    rng = np.random.default_rng(3)
    n = 37
    a = _frame(rng, n)
    S.same_frame(a, _copy(a))
    perm = rng.permutation(n)
    b = _moved(a, lambda v: S.permuted(v, perm))
    S.same_frame(a, b, rows=S.row_map(perm))
    S.same_frame(_moved(b, lambda v: S.unpermuted(v, perm)), a)
    with pytest.raises(AssertionError):
        S.same_frame(a, b)                                                   # the map left out
    # one float of one row, one ulp: every array in turn, and the message names array, gaussian and component
    for name in list(GRADS) + ["g2d"]:
        c = _copy(b)
        arr = c["g2d"] if name == "g2d" else c["grads"][name]
        flat = arr.reshape(n, -1)
        row, comp = 11, flat.shape[1] - 1
        flat.view(np.uint32)[row, comp] ^= 1
        with pytest.raises(AssertionError) as e:
            S.same_frame(a, c, rows=S.row_map(perm))
        want = f"{'g2d' if name == 'g2d' else 'd_' + name}: first difference at gaussian {int(perm[row])} (row {row} of the other frame), component {comp}"
        assert want in str(e.value), (want, str(e.value))
    for k in ("img", "tr"):
        c = _copy(b)
        c[k].reshape(-1).view(np.uint32)[5] ^= 1
        with pytest.raises(AssertionError, match=k):
            S.same_frame(a, c, rows=S.row_map(perm))
    c = _copy(b); c["grads"]["opacities"][4] = -0.0; a2 = _copy(a); a2["grads"]["opacities"][perm[4]] = 0.0
    with pytest.raises(AssertionError, match="d_opacities"):
        S.same_frame(a2, c, rows=S.row_map(perm))                           # - 0 is not + 0 here
    # the row map off by one
    with pytest.raises(AssertionError):
        S.same_frame(a, b, rows=np.roll(S.row_map(perm), 1))
    with pytest.raises(AssertionError):
        S.same_frame(a, b, rows=(S.row_map(perm) + 1) % n)
    # a tied pair that is NOT swapped passes: two rows with the same content, each compared with its own image
    d = _moved(a, lambda v: np.concatenate([v, v[-1:]]))                     # row n duplicates row n - 1
    perm2 = np.concatenate([rng.permutation(n - 1), [n - 1, n]])             # the pair keeps its order
    S.same_frame(d, _moved(d, lambda v: S.permuted(v, perm2)), rows=S.row_map(perm2))
    # a frame without g2d against one with it is refused, not skipped
    with pytest.raises((AssertionError, KeyError)):
        S.same_frame(a, _frame(np.random.default_rng(3), n, g2d=False))


def test_padded_keeps_the_live_rows_in_order():
    from gaussiansplat_amd import synthetic
    rng = np.random.default_rng(9)
    n = 500
    sc = synthetic.make_scene(n, 80, 56, 1, seed=3)
    for total in (n, n + 1, 768, 1025):
        pad, live, dead = S.padded(sc, total, rng)
        assert len(live) == n and np.all(np.diff(live) > 0)
        rows = np.concatenate([live] + list(dead.values()))
        assert np.array_equal(np.sort(rows), np.arange(total))               # every row is live or dead, none both
        for k, v in sc.items():
            assert pad[k].shape == (total,) + v.shape[1:] and same_bits(pad[k][live], v), k
        assert np.all(pad["means"][dead["offscreen"], :2] == np.float32(1e4)) and np.isfinite(pad["means"][dead["offscreen"], 2]).all()
        assert np.isnan(pad["means"][dead["nan"]]).all()
        for k in ("scales", "quats", "opacities", "shs"):                    # every other field is a live row's
            assert np.isfinite(pad[k]).all(), k
    if total > n + 10:
        assert all(len(v) > 0 for v in dead.values()) and not np.array_equal(live, np.arange(n))   # really in between, both kinds
    sc2 = synthetic.make_scene_2d(300, 100, 60, seed=2)
    pad, live, dead = S.padded(sc2, 512, rng)
    assert set(dead) == set(S.KINDS_2D) and np.all(np.diff(live) > 0)
    for k, v in sc2.items():
        assert same_bits(pad[k][live], v), k
    assert np.all(pad["opacities"][dead["transparent"]] == 0.0) and np.all(np.abs(pad["means"][dead["outside"]]) > 10.0)
    only = S.padded(sc, 600, rng, kinds=("offscreen",))[2]
    assert set(only) == {"offscreen"} and len(only["offscreen"]) == 100
    with pytest.raises(AssertionError):
        S.padded(sc, 600, rng, kinds=("transparent",))                       # a 2-D kind on a 3-D scene


def test_permuted_and_unpermuted_are_inverse():
    rng = np.random.default_rng(4)
    x = dict(a=rng.standard_normal((9, 3)).astype(np.float32), b=np.arange(9, dtype=np.int32))
    perm = rng.permutation(9)
    p = S.permuted(x, perm)
    assert np.array_equal(p["b"], perm)
    u = S.unpermuted(p, perm)
    assert all(same_bits(u[k], x[k]) for k in x)
    assert np.array_equal(np.asarray(p["b"])[S.row_map(perm)], x["b"])
    with pytest.raises(AssertionError):
        S.permuted(x, np.zeros(9, np.int64))
