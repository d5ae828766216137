"""The per-tile debug record of the composite kernels (gs_debug_tile_clock; GsCompositeArgs.tile_clock says what its 15 words mean).

Words 3 and 6 .. 14 are counts, not clocks, and on a frame where nothing freezes (t_min = 0) they have closed forms per tile: a tile with
w x h pixels inside the image (P = w h, A = ceil(h / 4) of its four 16 x 4 strips hold a pixel) that evaluates ev entries executes
4 ev strip slots, would need ev ceil(P / 64) with its pixels packed, has ev A strips and ev P pixels alive, and every evaluated entry
falls into one bin of each of the forward's three packing histograms.  On a dense frame with the early-out the words are bounded
by one another, and the forward must be seen to pack.  72 x 40 pixels: 5 x 3 tiles, the last column 8 wide, the last row 8 high;
one wave per tile, one binning round, records by tile in tile order (variant 10), alpha_cull on (the clock kernels refuse otherwise)."""
import numpy as np
import pytest

from common import halves

pytestmark = pytest.mark.gpu
N, W, H, DEG = 3000, 72, 40, 1
GX, GY = 5, 3
# log-scale shift of the dense frame.  Measured with the library of the commit before this test (d72859a): at 1.0 no pixel of this small
# scene freezes and no tile packs, at 2.0 thirteen of the fifteen tiles pack, at 3.0 all do and every tile stops before the end of its list
DENSE_GROW = 3.0


def _records(t_min, grow=0.0):
    from gaussiansplat_amd import backend as B, camera as gcam, synthetic
    sc = synthetic.make_scene(N, W, H, DEG, seed=77)
    scales = (sc["scales"] + np.float32(grow)).astype(np.float32)       # (grow > 0: the dense recipe of tests/test_gpu_caps.py)
    cam = synthetic.scene_camera(W, view=0)
    ctx = B.Context(t_min=t_min, tile_parts=1, slab_mode=0)           # (float atomics: the backward's clock kernels have no fixed-point form)
    ctx.set_model_host(sc["means"], scales, sc["quats"], sc["opacities"], sc["shs"].reshape(N, -1), DEG)
    ctx.set_camera(gcam.compute_transform(cam), gcam.compute_projection(cam, W, H), float(cam.fx), float(cam.fy), float(cam.near), float(cam.far),
                   cam.eye, cam.lookAt, W, H)
    ctx.preprocess(); ctx.bin()
    ctx.forward_host()
    ctx.backward(synthetic.make_dC(W, H, 7), ctx.grads_alloc(), overwrite=True)
    ranges = np.asarray(ctx.get_array(B.ARR_TILE_RANGES)).reshape(-1, 2).astype(np.int64)
    out = dict(listed=ranges[:, 1] - ranges[:, 0], wc=ctx.work_counters_ex(), fwd=ctx.tile_clock(0, 10), bwd=ctx.tile_clock(1, 10))
    ctx.close()
    assert out["fwd"].shape == out["bwd"].shape == (GX * GY, 15) and out["listed"].shape == (GX * GY,)
    return out


@pytest.fixture(scope="module")
def ragged():
    return _records(0.0)


@pytest.fixture(scope="module")
def dense():
    return _records(1e-5, grow=DENSE_GROW)


def _hists(clk):
    """[tiles, 3, 4]: the evaluated entries by the slots K = 1 .. 4 of the three packings (words 8 .. 13)"""
    h = np.zeros((clk.shape[0], 3, 4), np.int64)
    for w in range(3):
        h[:, w, 0], h[:, w, 1] = halves(clk[:, 8 + 2 * w])
        h[:, w, 2], h[:, w, 3] = halves(clk[:, 9 + 2 * w])
    return h


def _tile_geometry():
    t = np.arange(GX * GY)
    w = np.minimum(16, W - 16 * (t % GX)); h = np.minimum(16, H - 16 * (t // GX))
    return w, h, w * h, (h + 3) // 4


def test_forward_record_without_early_out_has_closed_forms(ragged):
    clk, listed = ragged["fwd"], ragged["listed"]
    w, h, P, A = _tile_geometry()
    walked, ev = halves(clk[:, 3])
    print("listed", listed, "ev", ev, "word14", clk[:, 14])
    assert listed.sum() > 0 and ev.sum() > 0
    assert np.array_equal(walked, listed)
    assert ev.sum() == ragged["wc"]["evaluated_fwd"]
    slots = (P + 63) // 64
    ex, ideal = halves(clk[:, 6])
    assert np.array_equal(ex, 4 * ev) and np.array_equal(ideal, ev * slots)
    alive, pix = halves(clk[:, 7])
    assert np.array_equal(alive, ev * A) and np.array_equal(pix, ev * P)
    want = np.zeros((GX * GY, 3, 4), np.int64)
    t = np.arange(GX * GY)
    want[t, 0, slots - 1] = ev; want[t, 1, A - 1] = ev; want[t, 2, A - 1] = ev
    assert np.array_equal(_hists(clk), want)
    bb = clk[:, 14].astype(np.int64)
    full = (w == 16) & (h == 16)
    assert full.sum() == 8 and np.array_equal(bb[full], ev[full])
    assert (bb <= listed).all()
    assert (clk[:, 0] <= clk[:, 1]).all()


def test_backward_record_without_early_out_matches_the_forward(ragged):
    f, b = ragged["fwd"], ragged["bwd"]
    ev = halves(f[:, 3])[1]
    assert np.array_equal(b[:, 3], f[:, 3])
    ex, ideal = halves(b[:, 6])
    print("backward strip slots", ex, "of", 4 * ev)
    assert (ex <= 4 * ev).all() and np.array_equal(ideal, halves(f[:, 6])[1])
    assert np.array_equal(b[:, 7], f[:, 7])


def test_forward_record_of_a_dense_frame_is_consistent_and_packs(dense):
    clk = dense["fwd"]
    walked, ev = halves(clk[:, 3])
    ex, ideal = halves(clk[:, 6])
    alive, pix = halves(clk[:, 7])
    print("listed", dense["listed"], "walked", walked, "ev", ev, "exec", ex, "ideal", ideal, "alive", alive, "pix", pix)
    assert ev.sum() > 0 and (walked < dense["listed"]).any()                   # pixels froze before their lists ended
    assert np.array_equal(_hists(clk).sum(axis=2), np.repeat(ev[:, None], 3, axis=1))
    assert (ideal <= ex).all() and (ex <= 4 * ev).all()
    assert (ideal <= alive).all() and (alive <= 4 * ev).all()
    assert (pix <= 64 * ideal).all()
    assert (ex < 4 * ev).any()                                                  # some tile ran packed
