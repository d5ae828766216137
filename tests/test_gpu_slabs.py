"""Binning in depth slabs (gs_config.slab_mode) must be invisible: same entries in the same order with the same 64-entry
batch boundaries as the classic single list, so image and transmittance are BIT-identical, deterministic-mode gradients
are BIT-identical, float-atomic gradients agree to atomic-order noise, and the oracle bars hold."""
import os

import numpy as np
import pytest

from common import GRADS, hip_context, one_wave_per_tile, rel_l2, run_frame, scene_and_cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_wave_per_tile(monkeypatch):
    one_wave_per_tile(monkeypatch)


# radix32 = (bin_path, rank_mode): the same frames on the 32-bit radix path (gs_bin2.hip), whose slab rounds drop the instances of
# completed tiles while ranking (ExpandArgs.done) and hand the second pass its key count on the device (live_total).  The second
# pass runs on grids of more than 256 tiles and a round has several chunks from 4096 instances on, so these cases take a larger image.
_SLAB_CASES = [((0.3,), 2), ((0.15, 0.5), 3), ((0.1, 0.2, 0.4), 4), ((0.999,), 2), ((0.0005, 0.6), 3)]
@pytest.mark.parametrize("fractions,rounds,radix32",
                         [pytest.param(f, r, None, id="fractions%d-%d" % (i, r)) for i, (f, r) in enumerate(_SLAB_CASES)] +      # (the ids these cases always had)
                         [pytest.param((0.15, 0.5), 3, (2, rm), id="bin2-rank%d" % rm) for rm in (0, 1)])
@pytest.mark.parametrize("t_min", [1e-3, 1e-5])
def test_forced_slabs_bit_identical_to_classic(oracle, fractions, rounds, radix32, t_min):
    from gaussiansplat_amd import synthetic
    O = oracle
    n, W, H, deg = 5000, 112, 72, 2                                          # ragged: 7 x 4.5 tiles
    path = {}
    if radix32:
        W, H = 280, 248                                                      # ragged: 17.5 x 15.5 tiles, 288 > 256
        path = dict(bin_path=radix32[0], rank_mode=radix32[1])
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 17)
    sc["scales"] = sc["scales"] + np.float32(1.2)                           # dense: several hundred entries per tile, pixels freeze
    dC = synthetic.make_dC(W, H, 17)
    res = {}
    for det in (True, False):
        c0 = hip_context(sc, cam, T, P, W, H, deg, order=1, t_min=t_min, deterministic=det, slab_mode=0, **path)
        r0 = run_frame(c0, dC, deg); c0.close()
        assert r0["rounds"] == 1
        c1 = hip_context(sc, cam, T, P, W, H, deg, order=1, t_min=t_min, deterministic=det, slab_mode=1, slab_fractions=fractions, **path)
        r1 = run_frame(c1, dC, deg)
        assert r1["rounds"] == rounds, r1["rounds"]
        if radix32:                                                          # not by falling back: several rounds, on the radix path, two passes, several chunks
            assert c1.num_rounds > 1 and c1.bin_path_of_frame() == 2, (c1.num_rounds, c1.bin_path_of_frame())
            assert ((W + 15) // 16) * ((H + 15) // 16) > 256 and c1.num_instances > 4096, c1.num_instances
        with pytest.raises(Exception):
            c1.get_array(13)                                                # lists are spread over the rounds
        c1.close()
        assert np.array_equal(r0["img"], r1["img"]) and np.array_equal(r0["tr"], r1["tr"])   # image, transmittance: bit-identical
        assert r1["tr"].min() >= 0.0                                                       # no sign flag left behind
        assert r0["wc"]["walked_fwd"] >= r1["wc"]["walked_fwd"] > 0 and r1["wc"]["walked_bwd"] == r1["wc"]["walked_fwd"]
        assert r1["wc"]["evaluated_fwd"] == r0["wc"]["evaluated_fwd"] == r1["wc"]["evaluated_bwd"]
        for k in GRADS:
            if det:
                assert np.array_equal(r0["grads"][k], r1["grads"][k]), k
            else:
                assert rel_l2(r1["grads"][k].reshape(-1), r0["grads"][k].reshape(-1)) <= 1e-5, k
        res[det] = r1
    if radix32:
        return                                                              # (the oracle bars below are this scene's on the small image: held by the cases above)
    ref = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=t_min)
    gref = O.backward(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, ref["ranges"], ref["ids"], dC, t_min=t_min)
    img, tr = res[False]["img"], res[False]["tr"]
    assert np.all(np.abs(img - ref["image"]) <= 1e-4 + 1e-4 * np.abs(ref["image"]))
    assert np.all(np.abs(tr - ref["trans"]) <= 1e-4 + 1e-4 * np.abs(ref["trans"]))
    for k in GRADS:
        assert rel_l2(res[False]["grads"][k].reshape(-1), gref[k].reshape(-1)) <= 1e-3, k


def test_auto_slabs_after_a_dense_frame():
    """Automatic mode: the first frames of a ctx are classic (no history); once a frame walked less than the threshold share
    of its instances the binning switches to slabs; every frame gives the same bits.  The shipped threshold is 0.03 (with the
    two-level binning slabs no longer pay at C5's 0.06); the test raises it to round 2's 0.15 (gs_config.slab_max_ratio) to exercise the switch, then
    checks that the same scene and the headline workload C3 (28 %) stay classic at the shipped threshold."""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 300_000, 800, 608, 3
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 77)
    sc["scales"] = sc["scales"] + np.float32(1.5)                           # dense: under 10 % of the instances are walked
    dC = synthetic.make_dC(W, H, 3)
    ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=1e-5, deterministic=True, slab_max_ratio=0.15)
    frames = [run_frame(ctx, dC, deg) for _ in range(4)]
    share = frames[0]["wc"]["walked_fwd"] / ctx.num_instances
    assert share < 0.15, share
    assert frames[0]["rounds"] == 1 and frames[-1]["rounds"] == 3, [f["rounds"] for f in frames]
    for f in frames[1:]:
        assert np.array_equal(f["img"], frames[0]["img"]) and np.array_equal(f["tr"], frames[0]["tr"])
        for k in GRADS:
            assert np.array_equal(f["grads"][k], frames[0]["grads"][k]), k
        assert f["wc"]["evaluated_fwd"] == frames[0]["wc"]["evaluated_fwd"]
    ctx.close()
    ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=1e-5, deterministic=True)
    again = [run_frame(ctx, dC, deg) for _ in range(3)]
    assert [f["rounds"] for f in again] == [1, 1, 1] and share > 0.03
    assert np.array_equal(again[-1]["img"], frames[0]["img"])
    ctx.close()
    n, W, H, deg = synthetic.CONFIGS["C3"]
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 1236)
    ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=1e-5)
    dC = synthetic.make_dC(W, H, 3)
    assert [run_frame(ctx, dC, deg)["rounds"] for _ in range(3)] == [1, 1, 1]
    ctx.close()


def test_sparse_scene_stays_classic():
    """No tile saturates (tiny footprints): the walked share is ~1, so the automatic mode never leaves the single round."""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 20000, 320, 208, 1
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 5)
    sc["scales"] = sc["scales"] - np.float32(1.5)
    dC = synthetic.make_dC(W, H, 5)
    ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=1e-5)
    rounds = [run_frame(ctx, dC, deg)["rounds"] for _ in range(4)]
    assert rounds == [1, 1, 1, 1], rounds
    ctx.close()


def test_slab_resume_with_negative_transmittance():
    """A live pixel's T can go (slightly) negative: rounding in the exponent of a near-singular, elongated, fully opaque splat
    can push alpha past 1.  Round 2 carried the `frozen` flag of a pixel in the sign of its stored T between slab rounds, so
    such a pixel was resumed as frozen; the flags now travel in per-tile lane masks.  Elongated splats with sigmoid(o) = 1:
    forced slabs must stay bit-identical to the classic single list, including the pixels whose T is negative."""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 6000, 160, 112, 0
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 23)
    sc = dict(sc)
    s = sc["scales"].copy()
    s[:, 0] += np.float32(3.0); s[:, 1:] -= np.float32(3.5)                  # needles: 600 : 1 axis ratios, conics close to singular
    sc["scales"] = s
    sc["opacities"] = np.full(n, 30.0, np.float32)                          # cusigmoid(30) rounds to 1.0f
    dC = synthetic.make_dC(W, H, 23)
    res = []
    for kw in (dict(slab_mode=0), dict(slab_mode=1, slab_fractions=(0.07, 0.3)), dict(slab_mode=1, slab_fractions=(0.01, 0.02, 0.5))):
        ctx = hip_context(sc, cam, T, P, W, H, deg, order=1, t_min=1e-5, deterministic=True, **kw)
        res.append(run_frame(ctx, dC, deg))
        ctx.close()
    assert res[0]["rounds"] == 1 and res[1]["rounds"] == 3 and res[2]["rounds"] == 4
    for r in res[1:]:
        assert np.array_equal(r["img"], res[0]["img"]) and np.array_equal(r["tr"], res[0]["tr"], equal_nan=True)
        for k in GRADS:
            assert np.array_equal(r["grads"][k], res[0]["grads"][k], equal_nan=True), k


def test_forced_slabs_with_super_tiles_of_16(oracle):
    """The slab rounds on the two-level path with super-tiles of 16 x 16 tiles (the default of 4K-class grids, forced here):
    completed super-tiles (super_done_kernel<4>) and completed tiles drop out of the later rounds; bits as with one round."""
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H, deg = 9000, 600, 392, 1                                         # 38 x 25 tiles: 3 x 2 super-tiles of 16, ragged
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 23)
    sc["scales"] = sc["scales"] + np.float32(1.3)
    dC = synthetic.make_dC(W, H, 23)
    c0 = hip_context(sc, cam, T, P, W, H, deg, order=1, t_min=1e-4, deterministic=True, slab_mode=0)
    r0 = run_frame(c0, dC, deg); c0.close()
    for flags in (B.GS_DEBUG_SUPER16, 0):
        c1 = hip_context(sc, cam, T, P, W, H, deg, order=1, t_min=1e-4, deterministic=True, slab_mode=1, slab_fractions=(0.12, 0.4), debug_flags=flags)
        r1 = run_frame(c1, dC, deg); c1.close()
        assert r1["rounds"] == 3
        assert np.array_equal(r0["img"], r1["img"]) and np.array_equal(r0["tr"], r1["tr"])
        assert r1["wc"]["walked_bwd"] == r1["wc"]["walked_fwd"] and r1["wc"]["evaluated_fwd"] == r0["wc"]["evaluated_fwd"] == r1["wc"]["evaluated_bwd"]
        for k in GRADS:
            assert np.array_equal(r0["grads"][k], r1["grads"][k]), k
