"""What a frame inherits from the frames before it, and what it must not (gs_ctx.h, "HISTORY").

Four things travel from frame to frame: the view slot's launch order, the slot's per-tile walk (list caps in gs_bin, list segments of the
small-grid backward), the ctx's walked share (slab rounds) and the order kernel's hand-off on the side stream.  The tests pin WHO inherits
WHAT: the same slot on the same grid does, another slot does not, another grid does not (in either direction), a slot-less frame does only
under schedule 4, and a frame abandoned after gs_bin leaves the walked share as a complete frame would.

The smallest frames at which history engages at all: 160 x 96 pixels (10 x 6 tiles), n = 3000, degree 1, the early-out on, deterministic.
Three configurations force the paths on with the test switches:
  CAPS      bin_path = 3 (two-level binning), list_cap = 2 (caps on small grids), GS_DEBUG_ALWAYS_ORDER (launch orders and the side stream on
            a small grid): the walk shows as capped lists (list_stats), the orders as gs_debug_tile_clock_rows > 0
  SEGMENTS  the defaults with automatic tile_parts: the slot's previous walk turns every tile's backward into two list segments, which shows
            as eight times the workgroups per pixel part (tile_clock_rows; tile_parts_of_frame stays 4)
  SLABS     bin_path = 3, slab_max_ratio = 0.15: a walked share below it shows as three binning rounds (num_rounds)
Each test first asserts that the history engaged, then the invariant.  Whole-tile frames (tile_parts = 1) are compared bit for bit with a
ctx that has no history; frames under automatic tile_parts, whose gradient bits depend on the history they ran on, with a ctx that has the
SAME history."""
import numpy as np
import pytest

from common import GRADS, hip_context, run_frame, same_bits, scene_and_cameras

pytestmark = pytest.mark.gpu

N, W, H, DEG = 3000, 160, 96, 1
ALWAYS_ORDER = 2                                                              # backend.GS_DEBUG_ALWAYS_ORDER
CAPS = dict(bin_path=3, list_cap=2, slab_mode=0, tile_parts=1, debug_flags=ALWAYS_ORDER)
SEGMENTS = dict(slab_mode=0, tile_parts=0)
SLABS = dict(bin_path=3, slab_mode=1, slab_max_ratio=0.15, list_cap=1, tile_parts=1)


@pytest.fixture(scope="module")
def scene():
    """(scene, T, P, camera, dC) -- dense, so that pixels freeze long before their lists end; read-only, shared by every test"""
    from gaussiansplat_amd import synthetic
    sc, cam, T, P, _ = scene_and_cameras(N, W, H, DEG, 41)
    sc["scales"] = (sc["scales"] + np.float32(2.0)).astype(np.float32)
    for a in sc.values():
        a.setflags(write=False)
    return sc, cam, T, P, synthetic.make_dC(W, H, 41)


@pytest.fixture(scope="module")
def dense_scene(scene):
    """the scene with every gaussian over most of the image and nearly opaque: a forward walks a few per cent of its list entries (slab rounds engage
    below 15 %; with the scene's own opacities it walks 18 %)"""
    sc = {k: v.copy() for k, v in scene[0].items()}
    sc["scales"] = (sc["scales"] + np.float32(1.5)).astype(np.float32)
    sc["opacities"] = (sc["opacities"] + np.float32(4.0)).astype(np.float32)
    return (sc,) + scene[1:]


def _ctx(scene, **kw):
    sc, cam, T, P, _ = scene
    return hip_context(sc, cam, T, P, W, H, DEG, t_min=1e-5, deterministic=True, **kw)


def _view(ctx, view, w=W, h=H):
    """camera `view` of the synthetic ring, on a w x h image"""
    from gaussiansplat_amd import camera as gcam, synthetic
    cam = synthetic.scene_camera(w, view=view)
    T = gcam.compute_transform(cam); P = gcam.compute_projection(cam, w, h)
    ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                   cam.eye, cam.lookAt, w, h)


def _frame(ctx, dC, slot=None):
    f = run_frame(ctx, dC, DEG, slot=slot)
    f["rows"] = ctx.tile_clock_rows()
    return f


def _same(a, b):
    assert same_bits(a["img"], b["img"]) and same_bits(a["tr"], b["tr"])
    for k in GRADS:
        assert same_bits(a["grads"][k], b["grads"][k]), k


def _fresh(scene, kw, view=0, frames=1, slot=None, w=W, h=H, dC=None):
    """the last of `frames` frames of a new ctx under one slot: a frame with exactly that much history"""
    ctx = _ctx(scene, **kw)
    _view(ctx, view, w, h)
    for _ in range(frames):
        f = _frame(ctx, scene[4] if dC is None else dC, slot)
    ctx.close()
    return f


@pytest.mark.parametrize("schedule,slot", [(3, 5), (4, None)])
def test_same_slot_same_grid_inherits_and_stays_invisible(scene, schedule, slot):
    """Frames 1 to 3 under one slot (schedule 4: of a ctx without slots): caps and the launch order engage from frame 2 -- the order kernel then
    runs on the side stream (GS_DEBUG_ALWAYS_ORDER) -- and every frame equals a ctx's first frame bit for bit."""
    dC = scene[4]
    first = _fresh(scene, dict(CAPS, schedule=schedule), slot=slot)
    assert not first["st"]["capped"] and first["rows"] > 0
    ctx = _ctx(scene, schedule=schedule, **CAPS)
    fs = [_frame(ctx, dC, slot) for _ in range(3)]
    ctx.close()
    assert [f["st"]["capped"] for f in fs] == [False, True, True] and all(f["rows"] > 0 for f in fs)
    for f in fs:
        _same(first, f)


def test_same_slot_segments_from_the_second_frame(scene):
    """Automatic tile_parts on a small grid: from the slot's second frame on the backward runs as list segments sized by the previous walk.  The
    gradient bits then depend on that walk, so a frame equals the frame of another ctx with the same history."""
    dC = scene[4]
    ctx = _ctx(scene, **SEGMENTS)
    fs = [_frame(ctx, dC, 5) for _ in range(3)]
    ctx.close()
    assert [f["parts"] for f in fs] == [4, 4, 4]
    assert fs[0]["rows"] > 0 and fs[1]["rows"] == fs[2]["rows"] == 8 * fs[0]["rows"], [f["rows"] for f in fs]   # 4 parts x 2 segments against 4 parts (an upper bound of both)
    _same(_fresh(scene, SEGMENTS, slot=9), fs[0])
    _same(_fresh(scene, SEGMENTS, slot=9, frames=2), fs[1])
    _same(_fresh(scene, SEGMENTS, slot=9, frames=3), fs[2])


def test_another_slot_inherits_nothing(scene):
    """Slot A (view 0), slot B (view 4), slot A again: B's first frame takes nothing from A -- full lists, no segments -- and A's later frame
    takes A's history."""
    dC = scene[4]
    for kw, engaged in ((CAPS, lambda f, f0: f["st"]["capped"]), (SEGMENTS, lambda f, f0: f["rows"] == 8 * f0["rows"])):
        ctx = _ctx(scene, **kw)
        _view(ctx, 0); a1 = _frame(ctx, dC, 3); a2 = _frame(ctx, dC, 3)
        _view(ctx, 4); b1 = _frame(ctx, dC, 4)
        _view(ctx, 0); a3 = _frame(ctx, dC, 3)
        ctx.close()
        assert not engaged(a1, a1) and engaged(a2, a1) and a1["rows"] > 0
        assert not engaged(b1, a1), (b1["st"], b1["rows"])
        assert engaged(a3, a1), (a3["st"], a3["rows"])
        _same(_fresh(scene, kw, view=4, slot=4), b1)
        _same(_fresh(scene, kw, view=0, slot=3, frames=3), a3)               # (A's third frame, as if B had never been rendered)


def test_grid_change_under_one_slot_inherits_nothing(scene):
    """160 x 96 -> 96 x 160 (the same 60 tiles, another grid key) -> 160 x 96 under one slot: nothing crosses the change in either direction, and
    the slot's history of the first grid is gone when the frame returns to it."""
    from gaussiansplat_amd import synthetic
    dC, dCt = scene[4], synthetic.make_dC(H, W, 41)
    for kw, engaged in ((CAPS, lambda f, f0: f["st"]["capped"]), (SEGMENTS, lambda f, f0: f["rows"] == 8 * f0["rows"])):
        ctx = _ctx(scene, **kw)
        g1 = [_frame(ctx, dC, 2) for _ in range(2)]
        _view(ctx, 0, H, W); g2 = [_frame(ctx, dCt, 2) for _ in range(2)]
        _view(ctx, 0, W, H); g3 = [_frame(ctx, dC, 2) for _ in range(2)]
        ctx.close()
        for g in (g1, g2, g3):
            assert g[0]["rows"] > 0 and not engaged(g[0], g[0]) and engaged(g[1], g[0]), [(f["st"], f["rows"]) for f in g]
        _same(_fresh(scene, kw, slot=2, w=H, h=W, dC=dCt), g2[0])
        _same(g1[0], g3[0]); _same(g1[1], g3[1])


def test_view_slot_changed_between_bin_and_forward(scene):
    """gs_set_view_slot between gs_bin and gs_forward: the lists were capped from the first slot's walk; the forward's order and the walk it
    leaves are the second slot's -- which has history from then on.  Bits as a ctx without history."""
    dC = scene[4]
    first = _fresh(scene, CAPS, slot=1)
    ctx = _ctx(scene, **CAPS)
    for _ in range(2):
        f = _frame(ctx, dC, 1)
    assert f["st"]["capped"] and f["rows"] > 0
    ctx.set_view_slot(1); ctx.preprocess(); ctx.bin()
    ctx.set_view_slot(2)
    img, tr = ctx.forward_host()
    st = ctx.list_stats()
    g = ctx.grads_alloc(); ctx.backward(dC, g)
    mixed = dict(img=img, tr=tr, grads=ctx.grads_read(g, DEG))
    assert st["capped"], st
    _same(first, mixed)
    s2 = _frame(ctx, dC, 2)                                                   # slot 2 was never bound during a gs_bin: its walk came from the mixed frame
    assert s2["st"]["capped"], s2["st"]
    _same(first, s2)
    s7 = _frame(ctx, dC, 7)                                                   # (a slot that was never bound at all)
    assert not s7["st"]["capped"]
    ctx.close()


@pytest.mark.parametrize("kw", [CAPS, SEGMENTS], ids=["caps", "segments"])
def test_slotless_frames_inherit_under_schedule_4_only(scene, kw):
    """Frames without a view slot: schedule 3 inherits nothing, ever; schedule 4 inherits from the ctx's previous slot-less frame."""
    dC = scene[4]
    engaged = (lambda f, f0: f["st"]["capped"]) if kw is CAPS else (lambda f, f0: f["rows"] == 8 * f0["rows"])
    out = {}
    for schedule in (3, 4):
        ctx = _ctx(scene, schedule=schedule, **kw)
        out[schedule] = fs = [_frame(ctx, dC) for _ in range(3)]
        with_slot = _frame(ctx, dC, 6)                                        # the slot-less frames are no slot's history
        ctx.close()
        assert fs[0]["rows"] > 0 and not engaged(with_slot, fs[0])
        assert [engaged(f, fs[0]) for f in fs] == ([False, False, False] if schedule == 3 else [False, True, True]), schedule
    _same(out[3][0], out[4][0])
    if kw is CAPS:                                                            # whole tiles: history is invisible
        _same(out[3][2], out[4][2])
    else:
        _same(_fresh(scene, dict(kw, schedule=3), slot=9, frames=3), out[4][2])   # schedule 4 without slots ran on what a slot would have kept


def test_frame_abandoned_after_bin_leaves_the_walked_share_alone(dense_scene):
    """gs_preprocess + gs_bin, then a new gs_preprocess before any gs_forward: the next complete frames choose their slab rounds (walked share
    below gs_config.slab_max_ratio = 0.15 -> three rounds) as they do with no abandoned frame in between, and give the same bits."""
    scene = dense_scene
    dC = scene[4]
    ref_ctx = _ctx(scene, **SLABS)
    ref = [_frame(ref_ctx, dC, 1) for _ in range(5)]
    ref_ctx.close()
    share = ref[0]["wc"]["walked_fwd"] / ref[0]["inst"]
    print("walked share", share, "rounds", [f["rounds"] for f in ref])
    assert share < 0.15 and ref[0]["rounds"] == 1 and ref[-1]["rounds"] == 3, (share, [f["rounds"] for f in ref])   # the share drives the rounds here
    ctx = _ctx(scene, **SLABS)
    got = [_frame(ctx, dC, 1) for _ in range(2)]
    ctx.set_view_slot(1); ctx.preprocess(); ctx.bin()                         # abandoned: binned, never rendered
    got += [_frame(ctx, dC, 1) for _ in range(3)]
    ctx.close()
    assert [f["rounds"] for f in got] == [f["rounds"] for f in ref], ([f["rounds"] for f in got], [f["rounds"] for f in ref])
    for a, b in zip(ref, got):
        _same(a, b)
        assert a["wc"] == b["wc"] and a["inst"] == b["inst"]
