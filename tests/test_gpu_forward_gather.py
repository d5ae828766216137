"""The forward walk's prefetch: the payload rows of the NEXT 64-entry batch are gathered into registers before the per-entry loops of the
current batch and first used behind them (gs_composite.hip: load_row / first_use_here).  The gathered rows must reach the staging of the
next batch whatever the loops in between did -- and lanes that gather nothing (a short last batch, a list that ends, a wave that stops)
must stay out of it.  The smallest frames on which that can go wrong:

  one        one gaussian: one entry, 63 lanes gather nothing;
  lengths    64 x 64 pixels, every gaussian inside ONE tile, so that the sixteen tile lists have exactly the lengths of LENGTHS: 1, one
             below / at / above one, two, three, four batches -- no batch, a one-entry batch, a full batch with nothing behind it;
  ragged     70 x 50: tiles cut by the right and the lower image edge;
  early      a dense frame on which pixels freeze batch by batch: the loops run with K = 4, then 2, then 1 slots per entry (seen in the
             debug clock's histogram), and waves stop with a gathered batch they never stage;
  caps       capped lists under a view slot whose history comes from another view, and the minimum cap on every tile: the waves append
             to their lists (extend_tile_list) and gather from what they appended;
  grid       81 x 64 = 5184 tiles, 20 k gaussians of a heavy-tailed scene under a view slot: launch order, split tiles, the SNAP forward.

Every case: image and transmittance against the CPU oracle with the same early-out (pixels |d| <= 1e-4 + 1e-4 |x|); the forward's work
counters equal to the backward's (where split tiles' backward runs as list segments: the walked counts); and the same bits from the variants that give the same bits by design --
  list_cap 0 / 1 / 2 and schedule 1 / 3: image, transmittance, deterministic gradients;
  tile_parts 1 / 2 with the no-op cull off: image, transmittance (with the cull on a wave drops entries that cannot reach ITS pixels);
  alpha_cull on / off: transmittance (the image to 2e-6 + 1e-6 |x|: what the no-op rule drops, tests/test_gpu_cull.py).
The oracle's early-out is itself checked, without a GPU, against its literal walk (t_min = 0: every entry of every list)."""
import functools

import numpy as np
import pytest

from common import GRADS, halves, hip_context, run_frame, scene_and_cameras

ALWAYS_ORDER = 2
T_MIN = 1e-5
LENGTHS = (1, 63, 64, 65, 127, 128, 129, 0, 2, 191, 192, 193, 255, 256, 257, 320)      # tile t of the 4 x 4 grid lists LENGTHS[t] entries
CASES = ("one", "lengths", "ragged", "early", "caps", "grid")


def _pix_ok(got, want):
    return bool(np.all(np.abs(got - want) <= 1e-4 + 1e-4 * np.abs(want)))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, cam, T, P, oracle camera, W, H, sh degree) -- built once, never modified"""
    from oracle import oracle as O
    if name == "one":
        W, H, deg = 48, 48, 1
        sc, cam, T, P, ocam = scene_and_cameras(1, W, H, deg, 5)
        sc["means"][:] = np.float32(0.0); sc["scales"][:] = np.float32(-1.5); sc["opacities"][:] = np.float32(2.0)
    elif name == "lengths":
        W, H, deg = 64, 64, 0
        cand, cam, T, P, ocam = scene_and_cameras(40_000, W, H, deg, 11)
        cand["scales"] = (cand["scales"] + np.float32(1.5)).astype(np.float32)
        cand["opacities"] = (cand["opacities"] * np.float32(0.5) - np.float32(2.0)).astype(np.float32)    # faint: no tile saturates
        r = O.render(cand["means"], cand["scales"], cand["quats"], cand["opacities"], cand["shs"], deg, ocam, order=1, t_min=T_MIN, omp=True)
        lists = np.bincount(r["ids"], minlength=40_000)                   # tile lists a candidate is in
        pick = []
        for t, want in enumerate(LENGTHS):                                  # the first `want` candidates that touch tile t and no other
            ids = np.sort(r["ids"][r["ranges"][t, 0]:r["ranges"][t, 1]])
            ids = ids[lists[ids] == 1]
            assert len(ids) >= want, (t, len(ids))
            pick.extend(ids[:want].tolist())
        pick = np.sort(np.asarray(pick, np.int64))
        sc = {k: np.ascontiguousarray(v[pick]) for k, v in cand.items()}
    elif name == "ragged":
        W, H, deg = 70, 50, 2
        sc, cam, T, P, ocam = scene_and_cameras(2_500, W, H, deg, 21)
        sc["scales"] = (sc["scales"] + np.float32(2.0)).astype(np.float32)
    elif name == "early":
        W, H, deg = 72, 40, 1                                               # the dense frame of tests/test_gpu_tile_clock.py: every tile packs and stops
        sc, cam, T, P, ocam = scene_and_cameras(3_000, W, H, deg, 77)
        sc["scales"] = (sc["scales"] + np.float32(3.0)).astype(np.float32)
    elif name == "caps":                                                    # the camera jump of tests/test_gpu_caps.py, seen from its far end (view 4)
        W, H, deg = 640, 480, 1
        sc, cam, T, P, ocam = scene_and_cameras(150_000, W, H, deg, 32, view=4)
        sc["scales"] = (sc["scales"] + np.float32(0.6)).astype(np.float32)
        far = sc["means"][:, 0] > np.quantile(sc["means"][:, 0], 0.66)      # a nearly transparent third: its tiles walk their whole lists
        sc["opacities"][far] = np.float32(-6.0)
    elif name == "grid":
        from gaussiansplat_amd import synthetic
        W, H, deg = 1296, 1024, 1                                           # 81 x 64 tiles: more than the chip's 5120 wave slots, so the frame gets a launch order
        _, cam, T, P, ocam = scene_and_cameras(16, W, H, deg, 1236)
        sc = synthetic.make_scene(20_000, W, H, deg, seed=1236, clustered=True)
    for v in sc.values():
        v.setflags(write=False)
    return sc, cam, T, P, ocam, W, H, deg


@functools.lru_cache(maxsize=None)
def _reference(name, t_min=T_MIN):
    from oracle import oracle as O
    O.build()
    sc, cam, T, P, ocam, W, H, deg = _case(name)
    r = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=t_min, omp=True)
    return dict(image=r["image"], trans=r["trans"], ranges=r["ranges"].astype(np.int64), instances=len(r["ids"]))


@pytest.mark.parametrize("name", CASES)
def test_oracle_early_out_stays_inside_its_literal_walk(name):
    """no GPU: the checker of the GPU tests below (t_min = 1e-5) against the walk as the reference writes it (t_min = 0)"""
    ref, lit = _reference(name), _reference(name, 0.0)
    assert ref["instances"] == lit["instances"] > 0
    assert _pix_ok(ref["image"], lit["image"]) and _pix_ok(ref["trans"], lit["trans"])
    if name == "lengths":
        assert tuple((ref["ranges"][:, 1] - ref["ranges"][:, 0]).tolist()) == LENGTHS
        assert 2_000 <= ref["instances"] <= 5_000
    if name == "early":                                                     # the early-out is at work: the literal walk goes on where pixels are frozen
        assert (lit["trans"] < T_MIN).mean() > 0.5


def _frame(ctx, dC, deg, slot=None, segments=False):
    """segments: heavy tiles' backward runs as list segments, each testing its entries against its OWN live rectangle: the walked counts agree,
    the evaluated counts need not (as on small grids, tests/test_gpu_parts.py)"""
    f = run_frame(ctx, dC, deg, slot=slot)
    assert f["wc"]["walked_fwd"] == f["wc"]["walked_bwd"] and (segments or f["wc"]["evaluated_fwd"] == f["wc"]["evaluated_bwd"]), f["wc"]
    return f


def _same_frames(a, b, grads=True):
    assert np.array_equal(a["img"], b["img"]) and np.array_equal(a["tr"], b["tr"])
    assert a["wc"] == b["wc"], (a["wc"], b["wc"])
    if grads:
        for k in GRADS:
            assert np.array_equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", CASES)
def test_forward_walk_prefetch(name):
    from gaussiansplat_amd import backend as B, synthetic
    sc, cam, T, P, ocam, W, H, deg = _case(name)
    ref = _reference(name)
    dC = synthetic.make_dC(W, H, 3)
    slot = 5 if name in ("caps", "grid") else None                          # (a view slot: list caps and launch orders come from its history)

    def run(frames=1, **kw):
        kw = dict(dict(t_min=T_MIN, deterministic=True, slab_mode=0, list_cap=1, tile_parts=1), **kw)
        ctx = hip_context(sc, cam, T, P, W, H, deg, **kw)
        out = [_frame(ctx, dC, deg, slot, segments=kw["tile_parts"] == 0) for _ in range(frames)]
        return ctx, out

    ctx, (base,) = run()
    assert base["inst"] == ref["instances"]
    assert np.array_equal(np.asarray(ctx.get_array(B.ARR_TILE_RANGES)).reshape(-1, 2).astype(np.int64), ref["ranges"])
    assert _pix_ok(base["img"], ref["image"]), np.abs(base["img"] - ref["image"]).max()
    assert _pix_ok(base["tr"], ref["trans"]), np.abs(base["tr"] - ref["trans"]).max()
    if name in ("one", "lengths"):
        assert base["wc"]["walked_fwd"] == ref["instances"]                  # nothing freezes: every list is walked to its end
    if name == "early":
        assert base["wc"]["walked_fwd"] < ref["instances"]
        h1, h2 = halves(ctx.tile_clock(0, 10)[:, 8])                        # evaluated entries while the live pixels fill 1 / 2 slots ...
        h3, h4 = halves(ctx.tile_clock(0, 10)[:, 9])                        # ... 3 / 4 slots (3: the walk stays at K = 4)
        assert h1.sum() > 0 and h2.sum() > 0 and h4.sum() > 0, (h1, h2, h3, h4)
    ctx.close()

    # alpha_cull off: the same transmittance, the image to what the no-op rule drops; the counters of the two kernels still agree
    ctx, (off,) = run(alpha_cull=False)
    ctx.close()
    assert np.array_equal(off["tr"], base["tr"])
    assert np.all(np.abs(off["img"] - base["img"]) <= 2e-6 + 1e-6 * np.abs(off["img"])), np.abs(off["img"] - base["img"]).max()
    assert off["wc"]["walked_fwd"] == base["wc"]["walked_fwd"] and off["wc"]["evaluated_fwd"] >= base["wc"]["evaluated_fwd"]

    # tile_parts 2, cull off: each wave walks the list for two of the four strips
    ctx, (two,) = run(alpha_cull=False, tile_parts=2)
    ctx.close()
    assert np.array_equal(two["img"], off["img"]) and np.array_equal(two["tr"], off["tr"])

    # list_cap 0 (automatic) and 2 (also on small grids), three frames each: from the second on a view slot's history caps the lists
    for cap in (0, 2):
        ctx, frames = run(frames=3, list_cap=cap, tile_parts=1)
        ctx.close()
        for f in frames:
            _same_frames(base, f)
        if name == "caps" and cap == 2:
            assert frames[1]["st"]["capped"] and frames[2]["st"]["capped"]

    # schedule 1 / 3 with launch orders also on these small grids
    res = {}
    for schedule in (1, 3):
        ctx, frames = run(frames=2, schedule=schedule, debug_flags=ALWAYS_ORDER)
        ctx.close()
        res[schedule] = frames[-1]
        _same_frames(base, frames[-1])
    _same_frames(res[1], res[3])

    if name == "caps":
        # (a) the minimum cap on every tile: every busy tile extends its list
        ctx, frames = run(frames=2, list_cap=0, debug_flags=B.GS_DEBUG_TINY_CAPS)
        ctx.close()
        for f in frames:
            assert f["st"]["capped"] and f["st"]["extended_segments"] > 0 and f["st"]["listed"] <= f["inst"], f["st"]
            _same_frames(base, f)
        # (b) a wrong history: the slot saw the scene from the other side (view 0), where the transparent third lies elsewhere
        camB = synthetic.scene_camera(W, view=0)
        ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=T_MIN, deterministic=True, slab_mode=0, list_cap=2, tile_parts=1)
        from gaussiansplat_amd import camera as gcam
        ctx.set_camera(gcam.compute_transform(camB), gcam.compute_projection(camB, W, H), float(np.float32(camB.fx)), float(np.float32(camB.fy)),
                       float(np.float32(camB.near)), float(np.float32(camB.far)), camB.eye, camB.lookAt, W, H)
        for _ in range(2):
            _frame(ctx, dC, deg, slot)
        ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                       cam.eye, cam.lookAt, W, H)
        jump = _frame(ctx, dC, deg, slot)
        ctx.close()
        assert jump["st"]["capped"] and jump["st"]["extended_segments"] > 0, jump["st"]
        _same_frames(base, jump)

    if name == "grid":
        # the production set-up: the second frame of a view slot runs on the slot's launch order, heavy tiles split into several waves
        # (their backward as list segments fed by the SNAP forward's snapshots); against whole tiles: the bars of tests/test_gpu_parts.py
        assert ref["ranges"].shape[0] > 5120
        ctx, frames = run(frames=2, list_cap=0, tile_parts=0)
        split = int((ctx.tile_clock(0, -30)[:2304, 1] > 0).sum())           # records of the order's front region: the extra waves of split tiles
        ctx.close()
        assert split >= 1, split
        f = frames[-1]
        assert _pix_ok(f["img"], ref["image"]) and _pix_ok(f["tr"], ref["trans"])
        assert np.abs(f["img"] - base["img"]).max() <= 1e-6 and np.abs(f["tr"] - base["tr"]).max() <= 1e-6
