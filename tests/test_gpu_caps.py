"""Capped tile lists (gs_config.list_cap; DESIGN.md "lists nobody walks") must be invisible.

gs_bin writes every tile's list only as far as the frame's view slot walked it last time (+ 25 % + 128 entries, rounded up to a
segment of the two-level binning); a composite wave that reaches the written end with live pixels appends the next segment of its
tile's list itself (gs_composite.hip: extend_tile_list).  Same entries, same order, same 64-entry batch boundaries as the full
lists, so: image and transmittance BIT-identical, deterministic-mode gradients BIT-identical, float-atomic gradients to atomic-order
noise, tile ranges the full ranges, and GS_ARR_SORTED_IDS / _KEYS (which first writes the unwritten rest) bit-exact vs the oracle.
Cases: history that is exact (no extension), a camera jump under a reused slot (extensions), the minimum cap on every tile
(GS_DEBUG_TINY_CAPS: every busy tile extends, incl. tiles that never saturate and walk their whole list), a grid with ragged
edges, slots beyond the old limit of 64, and the cap switched off."""
import numpy as np
import pytest

from common import GRADS, hip_context, one_wave_per_tile, rel_l2, run_frame, scene_and_cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_wave_per_tile(monkeypatch):
    one_wave_per_tile(monkeypatch)


def _set_cam(ctx, cam, W, H):
    from gaussiansplat_amd import camera as gcam
    T = gcam.compute_transform(cam); P = gcam.compute_projection(cam, W, H)
    ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                   cam.eye, cam.lookAt, W, H)


def _same_frames(a, b, det=True, oracle_grads=None):
    assert np.array_equal(a["img"], b["img"]) and np.array_equal(a["tr"], b["tr"])
    assert a["wc"]["walked_fwd"] == b["wc"]["walked_fwd"] == b["wc"]["walked_bwd"]
    assert a["wc"]["evaluated_fwd"] == b["wc"]["evaluated_fwd"] == b["wc"]["evaluated_bwd"]
    if det:
        for k in GRADS:
            assert np.array_equal(a["grads"][k], b["grads"][k]), k
        return
    # Float atomics: two runs of the SAME frame differ by the order of the additions.  Bars that do not follow what a run happened to
    # measure: (1) the per-gaussian 2-D sums, where the order noise is not amplified by the parameter chain, to 2e-6 --
    # fp32 sums of a few hundred terms each differ by ~1e-7 sqrt(terms) relative; (2) the parameter gradients: both runs inside the
    # oracle bar of 1e-3, and no further from each other than the worse of them is from the oracle.
    assert rel_l2(b["g2d"].reshape(-1), a["g2d"].reshape(-1)) <= 2e-6, rel_l2(b["g2d"].reshape(-1), a["g2d"].reshape(-1))
    for k in GRADS:
        d_ab = rel_l2(b["grads"][k].reshape(-1), a["grads"][k].reshape(-1))
        if oracle_grads is None:
            assert d_ab <= 1e-3, (k, d_ab)
            continue
        o = np.asarray(oracle_grads[k]).reshape(-1)
        d_ao, d_bo = rel_l2(a["grads"][k].reshape(-1), o), rel_l2(b["grads"][k].reshape(-1), o)
        assert d_ao <= 1e-3 and d_bo <= 1e-3, (k, d_ao, d_bo)
        assert d_ab <= max(d_ao, d_bo, 2e-6), (k, d_ab, d_ao, d_bo)


def _dense_scene(n, W, H, deg, seed, grow=1.0):
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, seed)
    sc["scales"] = (sc["scales"] + np.float32(grow)).astype(np.float32)     # dense: pixels freeze long before their lists end
    return sc, cam, T, P, ocam


@pytest.mark.parametrize("det", [True, False])
def test_capped_lists_from_slot_history_are_invisible(oracle, det):
    from gaussiansplat_amd import backend as B, synthetic
    O = oracle
    n, W, H, deg = 120_000, 648, 470, 2                                       # 41 x 30 tiles (ragged both ways), 6 x 4 super-tiles
    sc, cam, T, P, ocam = _dense_scene(n, W, H, deg, 31)
    dC = synthetic.make_dC(W, H, 31)
    plain = hip_context(sc, cam, T, P, W, H, deg, deterministic=det, list_cap=1, slab_mode=0)
    ref = run_frame(plain, dC, deg, slot=7, g2d=True)
    assert not ref["st"]["capped"] and ref["st"]["listed"] == ref["inst"]
    assert ref["wc"]["walked_fwd"] < 0.5 * ref["inst"]                         # the scene is dense enough for caps to matter
    og = None
    if not det:                                                                # the float-atomic runs are held against the oracle's adjoint
        o0 = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=1e-5, omp=True)
        og = O.backward(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, o0["ranges"], o0["ids"], dC, t_min=1e-5, omp=True)
    ctx = hip_context(sc, cam, T, P, W, H, deg, deterministic=det, list_cap=2, slab_mode=0)
    f1 = run_frame(ctx, dC, deg, slot=7, g2d=True)                             # no history yet: full lists
    assert not f1["st"]["capped"]
    _same_frames(ref, f1, det, og)
    for rep in range(3):                                                       # history from the same view: capped, nothing to extend
        f = run_frame(ctx, dC, deg, slot=7, g2d=True)
        assert f["st"]["capped"] and f["st"]["extended_segments"] == 0, f["st"]
        assert f["wc"]["walked_fwd"] <= f["st"]["listed"] < 0.8 * f["inst"], (f["st"], f["inst"], f["wc"])
        _same_frames(ref, f, det, og)
    # the full ranges are always there; asking for the ids writes the unwritten rest, and the frame still finishes
    ctx.set_view_slot(7); ctx.preprocess(); ctx.bin()
    oref = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=1e-5, omp=True)
    assert np.array_equal(ctx.get_array(B.ARR_TILE_RANGES), oref["ranges"])
    img, tr = ctx.forward_host()
    assert ctx.list_stats()["capped"]
    assert np.array_equal(ctx.get_array(B.ARR_SORTED_IDS), oref["ids"])
    assert np.array_equal(ctx.get_array(B.ARR_SORTED_KEYS), oref["keys"])
    assert not ctx.list_stats()["capped"]
    g = ctx.grads_alloc(); ctx.backward(dC, g)
    got = ctx.grads_read(g, deg)
    assert np.array_equal(img, ref["img"]) and np.array_equal(tr, ref["tr"])
    for k in GRADS:
        if det:
            assert np.array_equal(got[k], ref["grads"][k]), k
    # a frame under another slot has no history: full lists again
    f = run_frame(ctx, dC, deg, slot=2000, g2d=True)                           # (slots up to 4095: the old limit was 64)
    assert not f["st"]["capped"]
    _same_frames(ref, f, det, og)
    plain.close(); ctx.close()


def test_camera_jump_under_a_reused_slot_extends_lists_in_the_kernel():
    """The slot's history comes from another view: many tiles walk further than their cap.  The waves append what they need."""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 150_000, 640, 480, 1
    sc, cam, T, P, ocam = _dense_scene(n, W, H, deg, 32, grow=0.6)
    # the right third of the scene is made nearly transparent: those tiles never saturate and walk their whole lists in view A
    far = sc["means"][:, 0] > np.quantile(sc["means"][:, 0], 0.66)
    sc["opacities"][far] = np.float32(-6.0)
    dC = synthetic.make_dC(W, H, 32)
    camA = synthetic.scene_camera(W, view=0)
    camB = synthetic.scene_camera(W, view=4)                                   # from behind: the transparent third is on the other side
    ctx = hip_context(sc, cam, T, P, W, H, deg, deterministic=True, list_cap=2, slab_mode=0)
    plain = hip_context(sc, cam, T, P, W, H, deg, deterministic=True, list_cap=1, slab_mode=0)
    _set_cam(ctx, camA, W, H); _set_cam(plain, camA, W, H)
    a0 = run_frame(plain, dC, deg, slot=5, g2d=True)
    for _ in range(2):
        a = run_frame(ctx, dC, deg, slot=5, g2d=True)
        _same_frames(a0, a)
    assert a["st"]["capped"]
    _set_cam(ctx, camB, W, H); _set_cam(plain, camB, W, H)                     # the jump: slot 5 now shows view B
    b0 = run_frame(plain, dC, deg, slot=5, g2d=True)
    b = run_frame(ctx, dC, deg, slot=5, g2d=True)
    assert b["st"]["capped"] and b["st"]["extended_segments"] > 0, b["st"]
    _same_frames(b0, b)
    b2 = run_frame(ctx, dC, deg, slot=5, g2d=True)                             # the history has caught up
    assert b2["st"]["capped"] and b2["st"]["extended_segments"] == 0, b2["st"]
    _same_frames(b0, b2)
    ctx.close(); plain.close()


@pytest.mark.parametrize("n,W,H,deg,grow,super16", [(120_000, 648, 470, 2, 1.0, False), (120_000, 648, 470, 2, 1.0, True), (40_000, 256, 208, 3, 0.3, False),
                                                    (300, 96, 64, 0, 0.0, False)])
def test_minimum_caps_everywhere(oracle, n, W, H, deg, grow, super16):
    """GS_DEBUG_TINY_CAPS: every tile's list is written up to its first segment(s) only; every tile that walks further extends
    its list -- also the tiles that never saturate, which end up appending their whole list.  Bits as with full lists, and vs
    the oracle within the usual bars."""
    from gaussiansplat_amd import backend as B, synthetic
    O = oracle
    sc, cam, T, P, ocam = _dense_scene(n, W, H, deg, 33, grow=grow)
    dC = synthetic.make_dC(W, H, 33)
    oref = O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=1e-5, omp=True)
    gref = O.backward(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, oref["ranges"], oref["ids"], dC, t_min=1e-5, omp=True)
    for det in (True, False):
        plain = hip_context(sc, cam, T, P, W, H, deg, deterministic=det, list_cap=1, slab_mode=0)
        ref = run_frame(plain, dC, deg, g2d=True); plain.close()
        ctx = hip_context(sc, cam, T, P, W, H, deg, deterministic=det, slab_mode=0, debug_flags=B.GS_DEBUG_TINY_CAPS | (B.GS_DEBUG_SUPER16 if super16 else 0))
        for rep in range(2):
            f = run_frame(ctx, dC, deg, g2d=True)
            assert f["st"]["capped"]
            if n >= 40_000:
                assert f["st"]["extended_segments"] > 0
            assert f["st"]["listed"] <= f["inst"]
            _same_frames(ref, f, det, None if det else gref)
        ctx.close()
    assert np.all(np.abs(f["img"] - oref["image"]) <= 1e-4 + 1e-4 * np.abs(oref["image"]))
    assert np.all(np.abs(f["tr"] - oref["trans"]) <= 1e-4 + 1e-4 * np.abs(oref["trans"]))
    for k in GRADS:
        assert rel_l2(f["grads"][k].reshape(-1), gref[k].reshape(-1)) <= 1e-3, k


def test_caps_engage_by_default_only_on_large_grids_and_through_the_renderer_mirror():
    """Default list_cap = 0: on at 1080p once the camera's slot has history AND the ctx's previous frame walked under 15 % of its list
    entries (a dense scene); off at C3's 28 % (the write pass does not pay there: profiles/r04b_kernel_stats_C3*) and on a grid of fewer
    tiles than wave slots.  The Python mirror names the slot by camera.id.  Two cameras alternate, as in bench.py."""
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    n, W, H, deg = 400_000, 1920, 1080, 3
    sc = synthetic.make_scene(n, W, H, deg, seed=1236)
    sc["scales"] = (sc["scales"] + np.float32(1.0)).astype(np.float32)        # dense: under 15 % of the entries are walked
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True)
    rp = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, list_cap=1)
    dC = torch.as_tensor(synthetic.make_dC(W, H, 5)).cuda()
    cams = [synthetic.scene_camera(W, view=0), synthetic.scene_camera(W, view=4)]
    out = {}
    for rr, name in ((rp, "plain"), (r, "capped")):
        res = []
        for i in range(6):
            cam = cams[i % 2]
            R.resetGrads(rr)
            tps = R.preprocess(rr, cam); R.compactIdxs(rr); R.forward(rr, tps); R.backward(rr, dC)
            torch.cuda.synchronize()
            res.append((rr.imageData.cpu().numpy().copy(), rr.transmittance.cpu().numpy().copy(), rr.splatGrads.flat.cpu().numpy().copy(),
                        rr.ctx.list_stats(), rr.ctx.num_instances))
        out[name] = res
    for i in range(6):
        p, c = out["plain"][i], out["capped"][i]
        assert np.array_equal(p[0], c[0]) and np.array_equal(p[1], c[1]) and np.array_equal(p[2], c[2]), i
        assert not p[3]["capped"]
        assert c[3]["capped"] == (i >= 2), (i, c[3])                            # the slot's first frame has no history
        if i >= 2:
            assert c[3]["extended_segments"] == 0 and c[3]["listed"] < 0.6 * c[4], (c[3], c[4])
    assert out["capped"][5][3]["listed"] < 0.4 * out["capped"][5][4]
    dense_small = synthetic.make_scene(50_000, 640, 480, 1, seed=3)
    dense_small["scales"] = (dense_small["scales"] + np.float32(1.0)).astype(np.float32)
    small = R.getRenderer("GAUSSIAN_3D", (640, 480, 3), (16, 16), None, dense_small)
    for i in range(4):
        tps = R.preprocess(small, synthetic.scene_camera(640)); R.compactIdxs(small); R.forward(small, tps)
        assert not small.ctx.list_stats()["capped"]                             # 1200 tiles: fewer than wave slots
    n3, W3, H3, d3 = synthetic.CONFIGS["C3"]
    c3 = R.getRenderer("GAUSSIAN_3D", (W3, H3, 3), (16, 16), None, synthetic.make_scene(n3, W3, H3, d3, seed=1236))
    for i in range(4):
        tps = R.preprocess(c3, synthetic.scene_camera(W3)); R.compactIdxs(c3); R.forward(c3, tps)
        assert not c3.ctx.list_stats()["capped"]                                # 28 % of the entries walked: full lists


def test_capped_lists_meet_the_speculative_overflow_redo():
    """capped lists (list_cap = 2, view-slot history) on a frame whose lists outgrow the buffers they were enqueued against.
    The first forward runs on empty lists (and overwrites the slot's walked counts, the caps' source, with zeros); the redo must not
    take its caps from there.  Image, transmittance and deterministic gradients equal those of uncapped lists bit for bit, the redo
    lists in full (capped = False) and reports no stale extension count."""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 6000, 480, 352, 1
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 123)
    dC = synthetic.make_dC(W, H, 9)
    base = sc["scales"].copy()
    res = {}
    for cap in (1, 2):
        ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=1e-5, deterministic=True, list_cap=cap, tile_parts=1)
        out = []
        for shift in (0.0, 0.0, 1.8, 1.8):                                 # history, history, 30-fold growth (redo), settled again
            s2 = (base + np.float32(shift)).astype(np.float32)
            ctx.set_model_host(sc["means"], s2, sc["quats"], sc["opacities"], sc["shs"].reshape(n, -1), deg)
            ctx.set_view_slot(3)
            ctx.preprocess(); ctx.bin()
            img, tr = ctx.forward_host()
            g = ctx.grads_alloc(); ctx.backward(dC, g)
            out.append((img, tr, ctx.grads_read(g, deg), ctx.list_stats(), ctx.num_instances))
        res[cap] = out
        ctx.close()
    assert res[2][1][3]["capped"] and res[2][3][3]["capped"]              # the slot's history caps the lists of ordinary frames
    assert res[2][2][4] > 8 * res[2][1][4]                                 # the growth really outran the buffers
    assert not res[2][2][3]["capped"] and res[2][2][3]["extended_segments"] == 0 and res[2][2][3]["listed"] == res[2][2][4]
    for k in range(4):
        a, b = res[1][k], res[2][k]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
        for name in ("means", "scales", "quats", "opacities", "shs"):
            assert np.array_equal(a[2][name], b[2][name]), (k, name)
