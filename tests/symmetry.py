"""The row symmetries of a frame, written once (tests/test_symmetry_host.py, tests/test_gpu_symmetry.py).

A gaussian's result does not depend on which row of the model it occupies, how many rows the model has, or which rows sit beside it.  Two
transformations state that, and one comparison checks it bit for bit:

  permuted(scene, perm)      row i of the result is row perm[i] of the scene; unpermuted(arrays, perm) is its inverse on anything with n
                             rows on axis 0 (model arrays, gradients, ARR_GRAD2D, optimiser moments, per-gaussian feature triples)
  padded(scene, n_total...)  dead rows at random positions between the live ones, which keep their relative order
  same_frame(a, b, rows)     image, transmittance, every gradient array and g2d of two run_frame results, b's rows mapped onto a's

The one documented dependence on the row index is the tie rule: gaussians with equal depth keys are listed in index order (include/gsplat.h,
GS_ARR_SORT_IDXS; the reference's sortperm is stable).  The synthetic scenes contain a few equal keys, so every scene the symmetry tests run on
comes from distinct_key_scene, which removes them and asserts that it did.

A row is DEAD when it reaches no tile list.  In the oracle, which has no frustum cull, that is a mean far off screen or a NaN mean; a gaussian
far behind the camera is not dead there.  The 2-D renderer's dead rows are a centre far outside the image and an opacity of 0.  The latter
is listed: alpha == 0 changes no pixel, but the early-out is defined on list positions ("at every 64-entry batch boundary of its
tile's list"), so such a row is dead only in frames without the early-out (t_min = 0)."""
import ctypes as C

import numpy as np

from common import GRADS, same_bits, scene_and_cameras

KINDS_3D = ("offscreen", "nan")
KINDS_2D = ("outside", "transparent")


# ---------------------------------------------------------------- scenes without equal depth keys
def depth_keys(scene, deg, ocam, order):
    """the 32-bit depth keys of the scene under `order`: gso_depth_key of the oracle's tps[:, 2]"""
    from oracle import oracle as O
    pre = O.preprocess(scene["means"], scene["scales"], scene["quats"], scene["opacities"], scene["shs"], deg, ocam)
    key = O.lib().gso_depth_key
    return np.array([key(C.c_float(z), int(order)) for z in pre["tps"][:, 2]], np.uint32)


def _others_of_equal(keys, means, among):
    """of the rows `among` that share a key, all but one.  Which one stays is decided by CONTENT -- the smallest (x, y) bit pattern, the row
    index only between gaussians that agree in both -- so that the same gaussians move wherever their rows sit in the model."""
    among = np.asarray(among, np.int64)
    xy = np.ascontiguousarray(means[among, :2], np.float32).view(np.uint32).reshape(-1, 2)
    by_content = among[np.lexsort((among, xy[:, 1], xy[:, 0]))]
    _, first = np.unique(keys[by_content], return_index=True)
    others = np.ones(len(by_content), bool)
    others[first] = False
    return by_content[others]


def remove_ties(scene, deg, ocam, orders=(1, 2), rows=None, max_rounds=4096):
    """Wherever two gaussians share a depth key under one of `orders` (ocam: one camera or a list of them -- then in any of their views), all
    but one of them have their means[:, 2] moved to the next float32; repeated until every key is distinct under each order.  rows: a mask of
    the rows that count (default all; the dead rows of a padded model reach no list, so their keys do not matter).  Which gaussians move
    depends on their content alone, never on their rows.  Changes scene["means"] in place and returns how many nudges it took."""
    ocams = list(ocam) if isinstance(ocam, (list, tuple)) else [ocam]
    among = np.arange(scene["means"].shape[0]) if rows is None else np.nonzero(rows)[0]
    nudges = 0
    for _ in range(max_rounds):
        tied = np.unique(np.concatenate([_others_of_equal(depth_keys(scene, deg, c, o), scene["means"], among) for o in orders for c in ocams]))
        if tied.size == 0:
            break
        z = scene["means"][tied, 2]
        scene["means"][tied, 2] = np.nextafter(z, np.float32(np.inf), dtype=np.float32)
        nudges += int(tied.size)
    for o in orders:
        for c in ocams:
            keys = depth_keys(scene, deg, c, o)[among]
            assert np.unique(keys).size == keys.size, f"order {o}: {keys.size - np.unique(keys).size} equal depth keys are left"
    return nudges


def distinct_key_scene(n, W, H, deg, seed, boost=0.0, orders=(1, 2), view=0, more_views=()):
    """(scene, cam, T, P, ocam) of common.scene_and_cameras for `view`, the log-scales raised by `boost`, and no two gaussians with one depth key
    under any of `orders`, in `view` and in each of `more_views` -- asserted, so that a test can never run on ties by accident.  The arrays are
    read-only: one scene serves many tests."""
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, seed, view=view)
    sc = {k: np.array(v, np.float32) for k, v in sc.items()}
    if boost:
        sc["scales"] = (sc["scales"] + np.float32(boost)).astype(np.float32)
    remove_ties(sc, deg, [ocam] + [scene_and_cameras(1, W, H, deg, seed, view=v)[4] for v in more_views], orders)
    for a in sc.values():
        a.setflags(write=False)
    return sc, cam, T, P, ocam


# ---------------------------------------------------------------- the transformations
def _rows(x, fn):
    """fn on an array with rows on axis 0, or on every value of a dict of such arrays"""
    if isinstance(x, dict):
        return {k: fn(np.asarray(v)) for k, v in x.items()}
    return fn(np.asarray(x))


def permuted(scene, perm):
    """row i of the result is row perm[i] of `scene` (a dict of arrays or one array; n rows on axis 0)"""
    perm = np.asarray(perm, np.int64)
    assert np.array_equal(np.sort(perm), np.arange(len(perm))), "not a permutation"

    def one(a):
        assert a.shape[0] == len(perm), (a.shape, len(perm))
        return np.ascontiguousarray(a[perm])
    return _rows(scene, one)


def unpermuted(arrays, perm):
    """the inverse of permuted: row perm[i] of the result is row i of `arrays`"""
    perm = np.asarray(perm, np.int64)

    def one(a):
        assert a.shape[0] == len(perm), (a.shape, len(perm))
        out = np.empty_like(a)
        out[perm] = a
        return out
    return _rows(arrays, one)


def row_map(perm):
    """same_frame's `rows` for a permuted model: base row j sits in row row_map(perm)[j] of the permuted one"""
    perm = np.asarray(perm, np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def padded(scene, n_total, rng, kinds=None):
    """`scene` with n_total - n dead rows inserted at random positions; the live rows keep their relative order.  Returns (padded scene, live,
    dead): live[j] is the row that holds the scene's row j, dead[kind] the rows of that kind.  A dead row is a copy of a random live row but
    for what kills it -- 3-D: "offscreen" the mean (1e4, 1e4, z), "nan" a NaN mean; 2-D: "outside" a centre far outside the image (means are
    fractions of it), "transparent" opacity 0."""
    two_d = "rots" in scene
    kinds = tuple(kinds) if kinds is not None else (KINDS_2D if two_d else KINDS_3D)
    assert kinds and all(k in (KINDS_2D if two_d else KINDS_3D) for k in kinds), kinds
    n = scene["means"].shape[0]
    extra = int(n_total) - n
    assert extra >= 0, (n_total, n)
    is_dead = np.zeros(n_total, bool)
    is_dead[rng.choice(n_total, extra, replace=False)] = True
    live, dead_rows = np.nonzero(~is_dead)[0], np.nonzero(is_dead)[0]
    src = rng.integers(0, n, extra)
    kind_of = rng.integers(0, len(kinds), extra)
    out = {}
    for k, v in scene.items():
        v = np.asarray(v)
        a = np.empty((n_total,) + v.shape[1:], v.dtype)
        a[live] = v
        a[dead_rows] = v[src]
        out[k] = a
    dead = {}
    for i, kind in enumerate(kinds):
        r = dead_rows[kind_of == i]
        dead[kind] = r
        if kind == "offscreen":
            out["means"][r, 0] = out["means"][r, 1] = np.float32(1e4)
        elif kind == "nan":
            out["means"][r] = np.float32(np.nan)
        elif kind == "outside":
            out["means"][r] = np.float32(-50.0)
        elif kind == "transparent":
            out["opacities"][r] = np.float32(0.0)
    return out, live, dead


# ---------------------------------------------------------------- the comparison
def first_difference(a, b):
    """None where a and b are the same bits, else (row, component, a's value, b's value) of the first element that differs; a -0.0 differs
    from a +0.0 and a NaN from a NaN of other bits (common.same_bits)"""
    a, b = np.asarray(a), np.asarray(b)
    if same_bits(a, b):
        return None
    if a.shape != b.shape or a.dtype != b.dtype:
        return (-1, -1, (a.shape, a.dtype), (b.shape, b.dtype))
    word = "u%d" % a.dtype.itemsize
    n = a.shape[0]
    diff = np.ascontiguousarray(a).view(word).reshape(n, -1) != np.ascontiguousarray(b).view(word).reshape(n, -1)
    row = int(np.argmax(diff.any(axis=1)))
    comp = int(np.argmax(diff[row]))
    return (row, comp, a.reshape(n, -1)[row, comp], b.reshape(n, -1)[row, comp])


def frame_differences(a, b, rows=None, names=None):
    """what same_frame asserts, as a list of messages (empty: the frames are equal)"""
    out = []
    for k in ("img", "tr"):
        d = first_difference(a[k], b[k])
        if d is not None:
            out.append(f"{k}: first difference in row {d[0]} of axis 0, element {d[1]} of it: {d[2]!r} against {d[3]!r}")
    per_row = {f"d_{k}": (a["grads"][k], b["grads"][k]) for k in a["grads"]}
    assert set(a["grads"]) == set(b["grads"]), (sorted(a["grads"]), sorted(b["grads"]))
    if "g2d" in a or "g2d" in b:
        per_row["g2d"] = (a["g2d"], b["g2d"])
    for name, (x, y) in per_row.items():
        if names is not None and name not in names:
            continue
        y = np.asarray(y)
        d = first_difference(x, y if rows is None else y[np.asarray(rows, np.int64)])
        if d is not None:
            where = f"gaussian {d[0]}" + ("" if rows is None else f" (row {int(np.asarray(rows)[d[0]])} of the other frame)")
            out.append(f"{name}: first difference at {where}, component {d[1]}: {d[2]!r} against {d[3]!r}")
    return out


def same_frame(a, b, rows=None):
    """Two run_frame results hold the same bits: image, transmittance, every gradient array and g2d where present.  rows: b's rows mapped onto
    a's -- a's gaussian j sits in b's row rows[j] (row_map(perm) for a permuted model, `live` for a padded one).  A failure names the array,
    the first differing gaussian and the component."""
    bad = frame_differences(a, b, rows)
    assert not bad, "\n".join(bad)


def rows_all_zero(arr, rows):
    """every float of the given rows is zero (+0 or -0 alike: a zero fill and an empty sum may differ in the sign)"""
    a = np.asarray(arr)
    return bool(np.all(a.reshape(a.shape[0], -1)[np.asarray(rows, np.int64)] == 0.0))


__all__ = ["GRADS", "KINDS_2D", "KINDS_3D", "depth_keys", "remove_ties", "distinct_key_scene", "permuted", "unpermuted", "row_map", "padded",
           "first_difference", "frame_differences", "same_frame", "rows_all_zero"]
