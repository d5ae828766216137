"""A frame must not care where a gaussian's row sits in the model (run on the MI355X: pytest -m gpu).

Every other test of the suite holds one scene of one size to a reference's bar.  These tests need no bar: they run the SAME content twice,
with its rows somewhere else, and compare bit for bit (tests/symmetry.py; tests/test_symmetry_host.py shows that the oracle holds the
property on these very scenes).  All contexts are deterministic: float atomics are order dependent, which is not the subject here.

  A  permutation   with distinct depth keys the frame of the permuted model is the frame of the base model once rows are mapped back:
                   image, transmittance, tile ranges, sorted keys, sorted ids through the map, ARR_GRAD2D and all five parameter gradients.
                   Not for ORDER_INDEX and the 2-D renderer, where the index IS the order.
  B  padding       dead rows between the live ones (a mean far off screen, a NaN mean; 2-D: a centre far outside, opacity 0) change
                   nothing on the live rows, and a gaussian off screen has all-zero gradient rows, every float.  Totals n + 1, 3072, 4096,
                   4097 and 16 385 -- one past the small binning's limit, so the same content takes the other binning path (asserted).
                   A row with a NaN mean holds zeros or NaNs (0 * NaN in the chain), never a finite non-zero float: no stale row.
  C  sign         the gradients of -dC are the negated gradients of dC, bit for bit (+0 / -0 count as equal, nothing else does): every
                   operation on the path is odd in dC and round-to-nearest is symmetric, the fixed-point conversion included.
  D  channels      permuting the colour channels of the SH coefficients permutes the image's planes and leaves the transmittance alone.
                   Forward only: the backward's cdot is an ordered fma chain over the channels.

A and B run under every launch mode below, each case asserting that the mode it names engaged the way the mode's own tests assert it
(configurations of tests/test_gpu_history.py, test_gpu_parts.py, test_gpu_slabs.py, test_gpu_cull.py, test_gpu_bin_small.py), and printing it
(profiles/symmetry.log).  The frame-level calls beyond the plain frame follow: the fused and unfused optimiser steps, the backward in its
phases, the colour exchange over two views, feature maps, view depths and the density statistics.

Out of scope, because the row index is part of their definition:
  gs_backward_camera                     a fixed summation tree over the rows: the order of the additions follows the rows;
  gs_density_restructure, the MCMC moves the output order is defined by the input order;
  non-deterministic mode                 float atomics;
  anything that needs a second GPU.
The history modes (list segments, capped lists) and the forced slabs run on the dense scene only, where their own tests show that they
engage; the 2-D renderer runs the modes that exist without a depth order."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import symmetry as S
from common import GRADS, dev, hip_context, on_torch_stream, run_frame, same_bits
from test_gpu_history import CAPS, SEGMENTS

pytestmark = pytest.mark.gpu

SCENES = {"dense": (3000, 160, 96, 1, 41, 2.0), "sparse": (2999, 200, 120, 3, 7, 0.0)}      # n, W, H, degree, seed, scale boost
TOTALS = (1, 3072, 4096, 4097, 16385)                                                        # 1: n + 1
SMALL_BIN_MAX = 16384                                                                        # gs_bin_small.hip: the one-launch binning's largest model
T_MIN = 1e-5


@functools.lru_cache(maxsize=None)
def _scene(name, more_views=()):
    from gaussiansplat_amd import synthetic
    n, W, H, deg, seed, boost = SCENES[name]
    sc, cam, T, P, ocam = S.distinct_key_scene(n, W, H, deg, seed, boost, more_views=more_views)
    dC = synthetic.make_dC(W, H, seed)
    dC.setflags(write=False)
    return SimpleNamespace(name=name, sc=sc, cam=cam, T=T, P=P, n=n, W=W, H=H, deg=deg, seed=seed, dC=dC, kind="3d")


@functools.lru_cache(maxsize=None)
def _scene_2d():
    from gaussiansplat_amd import synthetic
    n, W, H = 900, 100, 60
    sc = synthetic.make_scene_2d(n, W, H)
    for a in sc.values():
        a.setflags(write=False)
    dC = synthetic.make_dC(W, H, 5)
    dC.setflags(write=False)
    return SimpleNamespace(name="2d", sc=sc, n=n, W=W, H=H, deg=0, seed=5, dC=dC, kind="2d")


def _variants(s, rng, totals=TOTALS, permute=True, kinds=None, listed_dead=False):
    """the transformed models of one scene: (label, scene, rows, to_base, rows that must be all zero, lists, rows with a NaN mean).  lists:
    the dead rows reach no tile list, so lists, counters and statistics are compared too.

    NARROWED, with the documented reason: the 2-D renderer's transparent rows ARE listed.  alpha == 0 changes no pixel and no other gaussian's
    gradient, but the early-out is defined on list positions -- "at every 64-entry batch boundary of its tile's list a pixel with T < t_min"
    stops (Early-out; GSO_EARLY_BATCH of oracle/gs_oracle.h) -- so a listed row moves the boundaries, in the oracle as on the
    device.  Such rows are dead only without the early-out: they come in one more variant of the frames with t_min = 0 (listed_dead), compared
    on image, transmittance and gradients."""
    out = []
    if permute:
        perm = rng.permutation(s.n)
        out.append(("permuted", S.permuted(s.sc, perm), S.row_map(perm), perm, np.zeros(0, np.int64), True, np.zeros(0, np.int64)))
    if s.kind == "2d":
        plan = [(t, ("outside",), True) for t in totals] + ([(4097, S.KINDS_2D, False)] if listed_dead else [])
    else:
        plan = [(t, kinds, True) for t in totals]
    for total, kinds_, lists in plan:
        total = s.n + 1 if total == 1 else total
        pad, live, dead = S.padded(s.sc, total, rng, kinds_)
        to_base = np.full(total, -1, np.int64)
        to_base[live] = np.arange(s.n)
        out.append((f"padded to {total} ({', '.join(f'{len(v)} {k}' for k, v in dead.items())})", pad, live, to_base,
                    dead["offscreen" if s.kind == "3d" else "outside"], lists, dead.get("nan", np.zeros(0, np.int64))))
    return out


# ---------------------------------------------------------------- the launch modes
def _mode(kw, check, frames=1, slot=None, phases=("all",), scenes=("dense", "sparse", "2d")):
    return SimpleNamespace(kw=kw, check=check, frames=frames, slot=slot, phases=phases, scenes=scenes)


def _path(want_small, want_large=None):
    def check(fs, n):
        want = want_small if (n <= SMALL_BIN_MAX or want_large is None) else want_large
        assert [f["path"] for f in fs] == [want] * len(fs), ([f["path"] for f in fs], want, n)
        return f"gs_get_bin_path {want} at {n} rows"
    return check


def _rank(probe):
    def check(fs, n):
        assert fs[0]["probe"] == probe and fs[0]["path"] == 1, (fs[0]["probe"], fs[0]["path"])
        return f"rank probe {probe} ({'LDS-atomic ranks in use' if probe == 0 else 'not run: ballots'}), radix path 1"
    return check


def _dsort(fs, n):
    assert fs[0]["path"] == 0, fs[0]["path"]                     # the two-level binning reads the global depth order the sort under test wrote
    return "two-level binning on the global depth order"


def _cull(on):
    def check(fs, n):
        wc = fs[0]["wc"]
        assert wc["evaluated_fwd"] == wc["evaluated_bwd"] and wc["walked_fwd"] == wc["walked_bwd"] > 0, wc
        assert (wc["evaluated_fwd"] < wc["walked_fwd"]) if on else (wc["evaluated_fwd"] == wc["walked_fwd"]), wc
        return f"evaluated {wc['evaluated_fwd']} of {wc['walked_fwd']} walked"
    return check


def _early_out(on):
    def check(fs, n):
        f = fs[0]
        assert (f["wc"]["walked_fwd"] <= f["inst"]) if on else (f["wc"]["walked_fwd"] == f["inst"]), (f["wc"], f["inst"])
        assert f["wc"]["walked_fwd"] > 0 and (on or f["parts"] == 1)
        return f"walked {f['wc']['walked_fwd']} of {f['inst']} entries"
    return check


def _parts(p):
    def check(fs, n):
        assert fs[0]["parts"] == p, fs[0]["parts"]
        return f"{p} waves per tile"
    return check


def _segments(fs, n):
    rows = [f["rows"] for f in fs]
    assert [f["parts"] for f in fs] == [4, 4, 4] and rows[0] > 0 and rows[1] == rows[2] == 8 * rows[0], ([f["parts"] for f in fs], rows)
    return f"workgroups per frame {rows}: list segments from frame 2"


def _caps(fs, n):
    assert [f["st"]["capped"] for f in fs] == [False, True, True] and all(f["rows"] > 0 for f in fs), [(f["st"], f["rows"]) for f in fs]
    return f"capped lists from frame 2, launch orders of {fs[0]['rows']} workgroups"


def _slabs(fs, n):
    assert fs[0]["rounds"] > 1, fs[0]["rounds"]
    return f"{fs[0]['rounds']} binning rounds"


def _phases(fs, n):
    """(nothing to query: the phases are the calls the frame made, one gs_backward_ex per entry of mode.phases)"""
    return "the backward in its phases"


HISTORY = ("dense",)
MODES = {
    "bin_path0": _mode(dict(bin_path=0), _path(3, 0)),
    "bin_path1": _mode(dict(bin_path=1), _path(1)),
    "bin_path2": _mode(dict(bin_path=2), _path(2)),
    "bin_path3": _mode(dict(bin_path=3), _path(0)),
    "rank_mode0": _mode(dict(bin_path=1, rank_mode=0), _rank(0), scenes=("dense", "sparse")),
    "rank_mode1": _mode(dict(bin_path=1, rank_mode=1), _rank(-1), scenes=("dense", "sparse")),
    "depth_sort1": _mode(dict(bin_path=3, depth_sort=1), _dsort, scenes=("dense", "sparse")),
    "depth_sort2": _mode(dict(bin_path=3, depth_sort=2), _dsort, scenes=("dense", "sparse")),
    "alpha_cull_on": _mode(dict(alpha_cull=True), _cull(True)),
    "alpha_cull_off": _mode(dict(alpha_cull=False), _cull(False)),
    "t_min0": _mode(dict(t_min=0.0), _early_out(False)),
    "t_min1e-5": _mode(dict(t_min=T_MIN), _early_out(True)),
    "tile_parts1": _mode(dict(tile_parts=1), _parts(1)),
    "tile_parts2": _mode(dict(tile_parts=2), _parts(2)),
    "tile_parts4": _mode(dict(tile_parts=4), _parts(4)),
    "tile_parts0_segments": _mode(SEGMENTS, _segments, frames=3, slot=5, scenes=HISTORY),
    "capped_lists_orders_side_stream": _mode(CAPS, _caps, frames=3, slot=5, scenes=HISTORY),
    "slabs": _mode(dict(slab_mode=1, slab_fractions=(0.3, 0.6)), _slabs, scenes=HISTORY),
    "phases_composite_params": _mode({}, _phases, phases=("composite", "params"), scenes=("dense", "sparse")),
    "phases_composite_sh_geom": _mode({}, _phases, phases=("composite", "params_sh", "params_geom"), scenes=("dense", "sparse")),
}


def kw_t_min(mode):
    return mode.kw.get("t_min", T_MIN)


def _ctx(s, sc, order, **kw):
    from gaussiansplat_amd import backend as B
    if s.kind == "2d":
        ctx = B.Context(order=B.ORDER_INDEX, **kw)
        ctx.set_model_2d_host(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"])
        ctx.set_image_size(s.W, s.H)
        return ctx
    return hip_context(sc, s.cam, s.T, s.P, s.W, s.H, s.deg, order=order, **kw)


def _frames(s, sc, order, mode):
    """the mode's frames of one model on a ctx of its own, everything read back, the ctx closed"""
    from gaussiansplat_amd import backend as B
    kw = dict(t_min=T_MIN, tile_parts=1, slab_mode=0, deterministic=True)
    kw.update(mode.kw)
    ctx = _ctx(s, sc, order, **kw)
    try:
        fs = []
        for _ in range(mode.frames):
            f = run_frame(ctx, s.dC, s.deg, slot=mode.slot, phases=mode.phases, kind=s.kind, g2d=True)
            f.update(rows=ctx.tile_clock_rows(), path=ctx.bin_path_of_frame(), probe=ctx.rank_probe_result)
            f["ranges"] = ctx.get_array(B.ARR_TILE_RANGES) if f["rounds"] == 1 else None    # (slab frames spread their lists over the rounds)
            f["ids"] = ctx.get_array(B.ARR_SORTED_IDS) if f["rounds"] == 1 else None
            f["keys"] = ctx.get_array(B.ARR_SORTED_KEYS) if f["rounds"] == 1 else None
            fs.append(f)
    finally:
        ctx.close()
    return fs


def _same_frames(s, base, got, rows, to_base, zero, lists, nan_rows, label):
    for k, (a, b) in enumerate(zip(base, got)):
        what = f"{label}, frame {k + 1}"
        if lists:
            assert a["inst"] == b["inst"] and a["wc"] == b["wc"] and a["st"] == b["st"] and a["rounds"] == b["rounds"], (what, a["inst"], b["inst"], a["wc"], b["wc"])
        try:
            S.same_frame(a, b, rows)
        except AssertionError as e:
            raise AssertionError(f"{what}:\n{e}") from None
        if lists and a["ranges"] is not None:
            assert same_bits(a["ranges"], b["ranges"]), f"{what}: tile ranges"
            assert same_bits(a["ids"], to_base[b["ids"]].astype(np.uint32)), f"{what}: sorted ids through the map"
            if s.kind == "3d":                                   # tile << 32 | depth key: no index in it
                assert same_bits(a["keys"], b["keys"]), f"{what}: sorted keys"
            else:                                                # ORDER_INDEX: the low word is the index
                assert same_bits(a["keys"] >> np.uint64(32), b["keys"] >> np.uint64(32)), f"{what}: tiles of the sorted keys"
        for name, arr in list(b["grads"].items()) + [("g2d", b["g2d"])]:
            assert S.rows_all_zero(arr, zero), f"{what}: {name} of a gaussian off screen is not all zero"
            # a NaN mean gives a zero or a NaN gradient (0 * NaN in the chain, and in the conversion ARR_GRAD2D is read back through), never a
            # finite one: a stale row would be finite and non-zero
            dead = np.asarray(arr).reshape(len(arr), -1)[nan_rows]
            assert np.all((dead == 0.0) | np.isnan(dead)), f"{what}: {name} of a gaussian with a NaN mean holds a finite non-zero float"


def _check_mode(name, s, order, permute):
    mode = MODES[name]
    rng = np.random.default_rng(s.seed + 100 * order)
    base = _frames(s, s.sc, order, mode)
    said = mode.check(base, s.n)
    if s.name == "dense" and kw_t_min(mode) > 0.0:                     # the dense scene has pixels for the early-out to freeze: T below t_min
        frozen = int((base[0]["tr"] < kw_t_min(mode)).sum())          # (walked counts whole 64-entry batches: it equals the instances on lists this short)
        assert frozen > 0, frozen
        said += f"; {frozen} pixels below t_min"
    assert all(np.any(v != 0.0) for v in base[-1]["grads"].values()) and float(base[-1]["tr"].min()) < 1.0       # a frame with content
    print(f"\nsymmetry[{s.name} order={order} {name}]: engaged: {said}; instances {base[0]['inst']}")
    for label, sc, rows, to_base, zero, lists, nan_rows in _variants(s, rng, permute=permute, listed_dead=mode.kw.get("t_min") == 0.0):
        got = _frames(s, sc, order, mode)
        said = mode.check(got, sc["means"].shape[0])
        print(f"  {label}: {said}")
        _same_frames(s, base, got, rows, to_base, zero, lists, nan_rows, f"{s.name} order={order} {name} {label}")


CASES_3D = [(m, sc) for m in MODES for sc in ("dense", "sparse") if sc in MODES[m].scenes]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mode,scene", CASES_3D)
def test_frame_under_permutation_and_padding(oracle, mode, scene, order):
    """symmetries A and B of the plain frame (and of the backward in its phases), one launch mode per case"""
    _check_mode(mode, _scene(scene), order, permute=True)


@pytest.mark.parametrize("mode", [m for m in MODES if "2d" in MODES[m].scenes])
def test_2d_frame_under_padding(mode):
    """symmetry B of the 2-D renderer (index order: a permutation is another image)"""
    _check_mode(mode, _scene_2d(), 0, permute=False)


# ---------------------------------------------------------------- C: sign, D: channels
def _negated_or_both_zero(a, b):
    """b == -a bit for bit, except that a zero may carry either sign on either side"""
    a, b = np.asarray(a), np.asarray(b)
    flipped = np.ascontiguousarray(a).view(np.uint32) ^ np.uint32(0x80000000)
    return bool(np.all((flipped == np.ascontiguousarray(b).view(np.uint32)) | ((a == 0.0) & (b == 0.0))))


@pytest.mark.parametrize("mode", ["tile_parts1", "tile_parts0_segments"])
def test_gradients_are_odd_in_dC(oracle, mode):
    s = _scene("dense")
    pos = _frames(s, s.sc, 1, MODES[mode])
    print(f"\nsymmetry[sign {mode}]: engaged: {MODES[mode].check(pos, s.n)}")
    neg = _frames(SimpleNamespace(**{**vars(s), "dC": -s.dC}), s.sc, 1, MODES[mode])
    MODES[mode].check(neg, s.n)
    for k, (a, b) in enumerate(zip(pos, neg)):
        assert same_bits(a["img"], b["img"]) and same_bits(a["tr"], b["tr"]), k
        for name, x, y in [(n_, a["grads"][n_], b["grads"][n_]) for n_ in GRADS] + [("g2d", a["g2d"], b["g2d"])]:
            assert np.any(x != 0.0), name
            if not _negated_or_both_zero(x, y):
                bad = S.first_difference(np.where(x == 0.0, np.float32(0.0), x), np.where(y == 0.0, np.float32(0.0), -y))
                raise AssertionError(f"frame {k + 1}: {name} of -dC is not the negated {name} of dC: gaussian {bad[0]}, component {bad[1]}: {bad[2]!r} against {bad[3]!r}")


@pytest.mark.parametrize("scene", ["dense", "sparse"])
def test_image_planes_follow_the_sh_channels(oracle, scene):
    s = _scene(scene)
    mode = MODES["tile_parts1"]
    base = _frames(s, s.sc, 1, mode)[0]
    print(f"\nsymmetry[channels {scene}]: engaged: {mode.check([base], s.n)}")
    for chan in ([1, 2, 0], [2, 1, 0]):
        sc = dict(s.sc); sc["shs"] = np.ascontiguousarray(s.sc["shs"][:, :, chan])
        got = _frames(s, sc, 1, mode)[0]
        assert same_bits(got["img"], base["img"][chan]), chan
        assert same_bits(got["tr"], base["tr"]), chan
        assert not same_bits(got["img"], base["img"])


# ---------------------------------------------------------------- frame-level calls beyond the plain frame
CALL_TOTALS = (1, 4097)
LR6 = (1e-3, 4e-3, 2e-3, 5e-2, 2.5e-3, 1.25e-4)
B1, B2, EPS = 0.9, 0.999, 1e-8
MODEL = ("means", "scales", "quats", "opacities", "shs")


def _rows_of(sc):
    return sc["means"].shape[0]


def _widths(s):
    return (3, 3, 4, 1, 3 * (s.deg + 1) ** 2)


class _Device:
    """a ctx on torch's stream whose model is five torch tensors: what the fused steps change can be read back"""

    def __init__(self, s, sc, **kw):
        import torch
        from gaussiansplat_amd import backend as B
        self.s, self.n = s, _rows_of(sc)
        self.model = [dev(np.asarray(sc[k]).reshape(self.n, w)) for k, w in zip(MODEL, _widths(s))]
        self.ctx = on_torch_stream(B.Context(order=1, t_min=T_MIN, deterministic=True, tile_parts=1, slab_mode=0, **kw))
        self.ctx.set_model_device(self.n, s.deg, [t.data_ptr() for t in self.model])
        self.view(s.cam, s.T, s.P)
        self.dC = dev(s.dC)
        torch.cuda.synchronize()

    def view(self, cam, T, P):
        self.ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                            cam.eye, cam.lookAt, self.s.W, self.s.H)

    def zeros(self):
        """(five zeroed device arrays of the gradients' shapes, their gs_grads)"""
        import torch
        from gaussiansplat_amd import backend as B
        ts = [torch.zeros((self.n, w), dtype=torch.float32, device="cuda") for w in _widths(self.s)]
        return ts, B.GsGrads(*(t.data_ptr() for t in ts))

    def forward(self):
        self.ctx.preprocess(); self.ctx.bin(); self.ctx.forward_device()

    def read(self, ts):
        import torch
        torch.cuda.synchronize()
        return [t.detach().cpu().numpy().copy() for t in ts]

    def model_scene(self):
        m = self.read(self.model)
        return dict(means=m[0], scales=m[1], quats=m[2], opacities=m[3].reshape(-1), shs=m[4].reshape(self.n, -1, 3))

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.ctx.close()


def _same_rows(base, got, rows, label):
    """dicts of per-gaussian arrays, got's rows mapped onto base's"""
    assert set(base) == set(got), (sorted(base), sorted(got))
    for k in base:
        d = S.first_difference(base[k], np.asarray(got[k])[rows])
        assert d is None, f"{label}: {k}: first difference at gaussian {d[0]} (row {int(rows[d[0]])}), component {d[1]}: {d[2]!r} against {d[3]!r}"


def _each_variant(s, run, totals=CALL_TOTALS, same=(), zero=(), untouched=None, label=""):
    """run(scene) -> dict of per-gaussian arrays (and, under the names in `same`, arrays and values that must not change at all); the base
    model against its permutation and its paddings.  zero: the arrays whose rows of gaussians off screen are all zero; untouched(scene) -> the
    dict of what such rows must still hold."""
    rng = np.random.default_rng(s.seed + 7)
    base = run(s.sc)
    for lab, sc, rows, to_base, off, _, _ in _variants(s, rng, totals=totals, kinds=("offscreen",)):
        got = run(sc)
        lab = f"{label} {lab}"
        for k in same:
            if isinstance(base[k], np.ndarray):
                assert same_bits(base[k], got[k]), f"{lab}: {k}"
            else:
                assert base[k] == got[k], (lab, k, base[k], got[k])
        _same_rows({k: v for k, v in base.items() if k not in same}, {k: v for k, v in got.items() if k not in same}, rows, lab)
        for k in zero:
            assert S.rows_all_zero(got[k], off), f"{lab}: {k} of a gaussian off screen is not all zero"
        if untouched is not None and len(off):
            for k, v in untouched(sc).items():
                assert same_bits(np.asarray(got[k])[off], np.asarray(v, np.float32).reshape(np.asarray(got[k]).shape)[off]), f"{lab}: {k} of a gaussian off screen changed"
        print(f"  {lab}: equal")
    return base


def _untie(d):
    """The step before moved the means, and a moved model has equal depth keys about as often as a drawn one (one pair in 3000).  So the model
    a step is about to render goes through symmetry.remove_ties, which decides by CONTENT which gaussian of a pair moves one ulp: the same
    gaussians on both sides of every comparison, wherever their rows sit.  Distinct keys are asserted in there, never assumed."""
    import torch
    from oracle import oracle as O
    s = d.s
    ocam = O.camera_from_arrays(s.T, s.P, np.float32(s.cam.fx), np.float32(s.cam.fy), np.float32(s.cam.near), np.float32(s.cam.far), s.cam.eye,
                                s.cam.lookAt, s.W, s.H)
    m = d.model_scene()
    keep = np.isfinite(m["means"]).all(axis=1) & (m["means"][:, 0] < 1e3)                # (dead rows reach no list: their keys do not matter)
    if S.remove_ties(m, s.deg, ocam, orders=(1,), rows=keep):
        d.model[0].copy_(torch.from_numpy(m["means"]))
        torch.cuda.synchronize()


@pytest.mark.parametrize("step", ["sgd", "adam", "adam_unfused"])
def test_optimiser_steps_travel_with_the_rows(oracle, step):
    """gs_backward_sgd, gs_backward_adam (fused) and gs_backward + gs_adam_step: after two steps the parameters and both moments are equal
    through the row map, and untouched for gaussians off screen (zero moments, the parameters' own bits)."""
    s = _scene("dense")

    def run(sc):
        d = _Device(s, sc)
        (mt, m), (vt, v), (gt, g) = d.zeros(), d.zeros(), d.zeros()
        for t in (1, 2):
            _untie(d)
            d.forward()
            if step == "sgd":
                d.ctx.backward_sgd(d.dC.data_ptr(), 1e-3)
            elif step == "adam":
                d.ctx.backward_adam(d.dC.data_ptr(), m, v, LR6, B1, B2, EPS, t)
            else:
                d.ctx.backward(d.dC.data_ptr(), g, overwrite=True)
                d.ctx.adam_step(g, m, v, LR6, B1, B2, EPS, t)
        out = dict(zip(MODEL, d.read(d.model)))
        if step != "sgd":
            out.update({f"exp_avg_{k}": a for k, a in zip(MODEL, d.read(mt))})
            out.update({f"exp_avg_sq_{k}": a for k, a in zip(MODEL, d.read(vt))})
        d.close()
        return out
    print(f"\nsymmetry[{step}]: two steps on the resident model")
    base = _each_variant(s, run, zero=() if step == "sgd" else [f"exp_avg_{k}" for k in MODEL] + [f"exp_avg_sq_{k}" for k in MODEL],
                         untouched=lambda sc: {k: np.asarray(sc[k]) for k in MODEL}, label=step)
    assert all(not same_bits(base[k], np.asarray(s.sc[k], np.float32).reshape(base[k].shape)) for k in MODEL)      # the steps moved every group


def _view_cameras(s, views):
    from gaussiansplat_amd import camera as gcam, synthetic
    cams = [synthetic.scene_camera(s.W, view=v) for v in views]
    return cams, [(c, gcam.compute_transform(c), gcam.compute_projection(c, s.W, s.H)) for c in cams]


def test_colour_exchange_over_two_views(oracle):
    """gs_color_grads_pack, gs_color_rows_pack and gs_sh_grads_from_views / _from_touched: per view the counts are equal and the dense and the
    packed rows are equal through the map; d_shs of both rebuilds is equal through the map (and both rebuilds agree)."""
    import torch
    from gaussiansplat_amd import distributed as D
    s = _scene("dense", more_views=(1,))
    cams, views = _view_cameras(s, (0, 1))
    records = D.view_records(cams, s.W, s.H)

    def run(sc):
        d = _Device(s, sc)
        n, words = d.n, (d.n + 31) // 32
        dense = torch.zeros((2, n, 3), dtype=torch.float32, device="cuda")
        bits = torch.zeros((2, words), dtype=torch.int32, device="cuda")
        rows = torch.zeros((2, n, 3), dtype=torch.float32, device="cuda")
        count = torch.zeros(2, dtype=torch.int64, device="cuda")
        _, g = d.zeros()
        for v, (cam, T, P) in enumerate(views):
            d.view(cam, T, P)
            d.forward()
            d.ctx.backward(d.dC.data_ptr(), g, overwrite=True)
            d.ctx.color_grads_pack(dense[v].data_ptr())
            d.ctx.color_rows_pack(None, n, bits[v].data_ptr(), rows[v].data_ptr(), count[v:].data_ptr())
        k3 = _widths(s)[4]
        from_views = torch.ones((n, k3), dtype=torch.float32, device="cuda")
        from_touched = torch.ones((n, k3), dtype=torch.float32, device="cuda")
        d.ctx.sh_grads_from_views(records, dense.data_ptr(), from_views.data_ptr(), overwrite=True)
        d.ctx.sh_grads_from_touched(records, bits.data_ptr(), rows.data_ptr(), n, from_touched.data_ptr(), overwrite=True)
        h_dense, h_bits, h_rows, h_count, a, b = d.read([dense, bits, rows, count, from_views, from_touched])
        d.close()
        out = dict(d_shs_from_views=a, d_shs_from_touched=b)
        assert same_bits(a, b)
        for v in range(2):
            touched = np.nonzero(np.unpackbits(h_bits[v].view(np.uint8), bitorder="little")[:n])[0]
            assert len(touched) == int(h_count[v]) and 0 < len(touched) <= n, (len(touched), h_count[v])
            unpacked = np.zeros((n, 3), np.float32)
            unpacked[touched] = h_rows[v, :len(touched)]
            out[f"view{v}_dense"] = h_dense[v]
            out[f"view{v}_unpacked"] = unpacked
            out[f"view{v}_count"] = int(h_count[v])
        return out
    print("\nsymmetry[colour exchange]: two views")
    names = [f"view{v}_{k}" for v in range(2) for k in ("dense", "unpacked")]
    base = _each_variant(s, run, same=("view0_count", "view1_count"), zero=names + ["d_shs_from_views", "d_shs_from_touched"], label="colour exchange")
    assert base["view0_count"] > s.n // 4 and np.any(base["d_shs_from_views"] != 0.0)
    assert not same_bits(base["view0_dense"], base["view1_dense"])


def test_feature_maps_and_their_gradients(oracle):
    """gs_render_features and gs_backward_features with a per-gaussian triple that travels with its row"""
    import torch
    s = _scene("dense")
    rng = np.random.default_rng(3)
    feat0 = rng.uniform(-1.0, 2.0, (s.n, 3)).astype(np.float32)
    dF = dev(rng.standard_normal((3, s.H, s.W)).astype(np.float32))

    def run(sc):
        d = _Device(s, sc)
        n = d.n
        feat = np.zeros((n, 3), np.float32)
        live = np.isfinite(sc["means"]).all(axis=1) & (np.asarray(sc["means"])[:, 0] < 1e3)
        # the triple travels with its row: found through the one field no two live gaussians share
        order = {z.tobytes(): i for i, z in enumerate(np.asarray(s.sc["means"]))}
        src = np.array([order.get(z.tobytes(), -1) for z in np.asarray(sc["means"])])
        assert np.all(src[live] >= 0) and len(set(src[live])) == s.n
        feat[live] = feat0[src[live]]
        feat[~live] = 5.0
        f = dev(feat)
        d.forward()
        out = torch.full((3, s.H, s.W), -7.0, dtype=torch.float32, device="cuda")
        tr = torch.full((s.H, s.W), -7.0, dtype=torch.float32, device="cuda")
        d.ctx.render_features(f.data_ptr(), out.data_ptr(), tr.data_ptr())
        gt, g = d.zeros()
        d_feat = torch.full((n, 3), 9.0, dtype=torch.float32, device="cuda")
        d.ctx.backward_features(f.data_ptr(), out.data_ptr(), dF.data_ptr(), d_feat.data_ptr(), g)
        h = d.read([out, tr, d_feat] + gt[:4])
        d.close()
        res = dict(features=h[0], trans=h[1], d_feat=h[2])
        res.update({f"d_{k}": a for k, a in zip(MODEL[:4], h[3:])})
        return res
    print("\nsymmetry[feature maps]")
    base = _each_variant(s, run, same=("features", "trans"), zero=["d_feat"] + [f"d_{k}" for k in MODEL[:4]], label="feature maps")
    assert np.any(base["features"] != 0.0) and all(np.any(base[k] != 0.0) for k in ("d_feat", "d_means", "d_scales", "d_quats", "d_opacities"))


def test_view_depth_and_its_backward(oracle):
    """gs_view_depth and gs_view_depth_backward: z and d_means travel with their rows (dz is drawn per gaussian, from its depth's bits)"""
    s = _scene("dense")

    def run(sc):
        import torch
        d = _Device(s, sc)
        z = torch.full((d.n,), -1.0, dtype=torch.float32, device="cuda")
        d.ctx.view_depth(z.data_ptr())
        hz = d.read([z])[0]
        dz = ((hz.view(np.uint32) % np.uint32(1000)).astype(np.float32) - np.float32(499.5)) / np.float32(250.0)
        dz[~np.isfinite(hz)] = 0.0
        dm = torch.zeros((d.n, 3), dtype=torch.float32, device="cuda")
        d.ctx.view_depth_backward(dev(dz).data_ptr(), dm.data_ptr())
        out = dict(z=hz, d_means=d.read([dm])[0])
        d.close()
        keep = np.isfinite(np.asarray(sc["means"])).all(axis=1)
        out["z"] = np.where(keep, out["z"], np.float32(0.0))                             # (which NaN a NaN mean gives is left open)
        return out
    print("\nsymmetry[view depth]")
    base = _each_variant(s, run, label="view depth", totals=(1, 4097))
    assert np.unique(base["z"]).size > s.n // 2 and np.any(base["d_means"] != 0.0)


def test_density_statistics_and_decisions(oracle):
    """gs_density_accumulate over the frame, gs_density_decide and gs_density_plan: statistics and actions are equal through the map; the plan's
    counts are equal under a permutation and are the counts of the actions under a padding"""
    import density_ref as DR
    import torch
    from gaussiansplat_amd import backend as B
    from gaussiansplat_amd.density import density_params
    s = _scene("dense")
    p = density_params(scene_extent=4.0, grad_threshold=2e-4, percent_dense=0.012, min_opacity=0.1, max_world_fraction=0.5, max_extent_px=60)
    plans = []

    def run(sc):
        d = _Device(s, sc)
        n = d.n
        gs = torch.zeros(n, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        ext = torch.zeros(n, dtype=torch.int32, device="cuda")
        st = B.GsDensityStats(gs.data_ptr(), cnt.data_ptr(), ext.data_ptr())
        _, g = d.zeros()
        d.forward()
        d.ctx.backward(d.dC.data_ptr(), g, overwrite=True)
        d.ctx.density_accumulate(st)
        action = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        d.ctx.density_decide(st, p, action.data_ptr())
        plan = d.ctx.density_plan(action.data_ptr())
        h = d.read([gs, cnt, ext, action])
        d.close()
        assert plan == DR.counts(h[3]), (plan, DR.counts(h[3]))
        plans.append((n, plan))
        return dict(grad_sum=h[0], count=h[1], max_extent=h[2], action=h[3])
    print("\nsymmetry[density]")
    base = _each_variant(s, run, zero=("grad_sum", "count", "max_extent"), label="density")
    assert plans[0][1] == plans[1][1] and plans[1][0] == s.n, plans[:2]                  # (the second run is the permuted model)
    print("  plan (survivors, clones, splits, pruned):", plans[0][1])
    assert len(np.unique(base["action"])) >= 2, plans[0]                                 # a decision with several classes
    assert np.mean(base["grad_sum"] > 0) > 0.3 and base["count"].max() == 1
