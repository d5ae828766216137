"""The zero fills at the end of the composite launches' grids: the forward's appended workgroups clear the 2-D gradient rows,
the backward's the SH gradient rows of an overwriting backward.  Every case runs a ctx with the fills (the default) and a twin with
GS_DEBUG_NO_TAIL_FILL (the in-line forms), same seed, same calls: image and T bit for bit, deterministic gradients bit for bit,
float-atomic gradients within the bar test_gpu_schedule.py sets for two launches of the same frame (rel-L2 <= 1e-5)."""
import numpy as np
import pytest

from common import bits, hip_context, rel_l2, same_bits, scene_and_cameras

pytestmark = pytest.mark.gpu
NO_TAIL_FILL = 32                      # GS_DEBUG_NO_TAIL_FILL
ATOMIC_BAR = 1e-5                      # test_gpu_schedule.py: float-atomic gradients of two launches of the same frame
# 2-D model: log-scales U[0, 1) as the reference draws them (splat.jl:74-87; footprints of a few pixels).  With U[0, 3) (footprints of a
# hundred pixels: thousands of float atomics per row, and a rotation gradient that is a difference of large moments) two runs of the SAME
# code already differ by 1.1e-5 in d_rotations -- seen on a ctx's first frame, where both twins run the in-line fill: the bar is for order noise
# of sums of this size, as in test_gpu_schedule.py's scenes.  Measured, largest rel-L2 of four twin runs: 6.3e-6 at U[0, 3), 9.4e-7 at U[0, 2),
# 1.5e-7 at U[0, 1); the 3-D cases of this file: at most 1.5e-6.
SCALE_HI_2D = 1.0


def assert_same(out, ref, det, what):
    """out / ref: lists of frames; a frame = (image, T, grads dict or None)"""
    assert len(out) == len(ref)
    for f, (o, r) in enumerate(zip(out, ref)):
        assert same_bits(o[0], r[0]) and same_bits(o[1], r[1]), (what, f, "image / T")
        if o[2] is None:
            assert r[2] is None
            continue
        for k in o[2]:
            if det:
                assert same_bits(o[2][k], r[2][k]), (what, f, k)
            else:
                assert rel_l2(o[2][k].reshape(-1), r[2][k].reshape(-1)) <= ATOMIC_BAR, (what, f, k)


def set_cam(ctx, cam, T, P, W, H):
    ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                   cam.eye, cam.lookAt, W, H)


def frame(ctx, dC, g, deg, overwrite=True, log=None):
    ctx.preprocess(); ctx.bin()
    img, tr = ctx.forward_host()
    ctx.backward(dC, g, overwrite=overwrite)
    if log is not None:
        log.append(ctx.tail_fill_blocks())
    return img, tr, ctx.grads_read(g, deg)


def blocks(nbytes):
    return -(-nbytes // 32768)             # GS_TAIL_FILL_BYTES per fill workgroup


def carried(fills, n, k3, det, first=True):
    """the fill workgroups of a ctx's frames, all overwriting backwards: the forward's from the ctx's second frame on (the first finds no
    gradient rows to clear yet), the backward's on every frame"""
    fwd, bwd = blocks(n * 16 * (8 if det else 4)), blocks(n * k3 * 4)
    want = [(0 if first and f == 0 else fwd, bwd) for f in range(len(fills))]
    assert fills == want, (fills, want)


def both(script, det, **kw):
    """script(ctx) -> frames, on a ctx with the fills and on its twin without; returns the former's frames after comparing"""
    flags = kw.pop("debug_flags", 0)
    outs, fills = [], []
    for extra in (0, NO_TAIL_FILL):
        ctx = script.make(deterministic=det, debug_flags=flags | extra, **kw)
        script.log = []
        outs.append(script(ctx))
        fills.append(script.log)
        ctx.close()
    assert_same(outs[0], outs[1], det, script.__name__)
    assert all(f == (0, 0) for f in fills[1]), fills[1]        # the twin carried no fill
    script.fills = fills[0]                                     # (forward, backward) fill workgroups per logged frame
    return outs[0]


def scene(n, W, H, deg, seed, scale_shift=0.0, view=0):
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, seed, view=view)
    sc["scales"] = sc["scales"] + np.float32(scale_shift)
    return sc, cam, T, P


@pytest.mark.parametrize("det", [True, False])
def test_launch_order_path(det):
    """frames 2 and 3 of a view slot launch over an order (with its holes): the fill workgroups sit behind order_len"""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 20_000, 400, 304, 2
    sc, cam, T, P = scene(n, W, H, deg, 31, 0.6)
    dC = synthetic.make_dC(W, H, 31)

    def script(ctx):
        ctx.set_view_slot(5)
        g = ctx.grads_alloc()
        out = []
        for _ in range(3):
            out.append(frame(ctx, dC, g, deg, log=script.log))
            assert ctx.tile_clock_rows() >= 25 * 19             # the frame has a launch order (its entries, holes included)
        return out
    script.make = lambda **kw: hip_context(sc, cam, T, P, W, H, deg, **kw)
    both(script, det, debug_flags=2, slab_mode=0)               # GS_DEBUG_ALWAYS_ORDER: the grid is smaller than the wave slots
    carried(script.fills, n, 3 * (deg + 1) ** 2, det)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("tile_parts", [2, 4, 0])
def test_small_ragged_grid(det, tile_parts):
    """7 x 5 tiles, ragged edges, the two-level path (gs_bin clears no rows): 2 and 4 waves per tile, and (automatic, frames 2 and 3 of the
    slot) the backward as list segments -- the fill workgroups sit behind len x parts and behind the segment units"""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 2500, 100, 70, 3
    sc, cam, T, P = scene(n, W, H, deg, 7, 0.5)
    dC = synthetic.make_dC(W, H, 7)
    parts, rows = [], []

    def script(ctx):
        ctx.set_view_slot(0)
        g = ctx.grads_alloc()
        out = []
        for _ in range(3):
            out.append(frame(ctx, dC, g, deg, log=script.log))
            parts.append(ctx.tile_parts_of_frame())
            rows.append(ctx.tile_clock_rows())
            assert ctx.bin_path_of_frame() == 0                  # two-level lists: gs_bin cleared no gradient rows
        return out
    script.make = lambda **kw: hip_context(sc, cam, T, P, W, H, deg, **kw)
    both(script, det, bin_path=3, tile_parts=tile_parts)
    assert parts[:3] == [tile_parts or 4] * 3, parts
    # workgroups of the launches: 40 (7 x 5 tiles rounded to eight) x pixel parts; frames 2 and 3 of the automatic choice: x list segments
    seg = 8 if tile_parts == 0 else 1
    assert rows[:3] == [40 * parts[0], 40 * parts[0] * seg, 40 * parts[0] * seg], rows
    carried(script.fills, n, 3 * (deg + 1) ** 2, det)


@pytest.mark.parametrize("n,deg", [(1, 3), (3, 3), (257, 1), (1001, 3)])
def test_sizes(n, deg):
    """the SH slice of the flat gradient buffer starts at 44 n bytes: no multiple of 16 for odd n (head and tail of the fill)"""
    from gaussiansplat_amd import synthetic
    W, H = 64, 48
    sc, cam, T, P = scene(n, W, H, deg, 11 + n, 0.8)
    dC = synthetic.make_dC(W, H, 3)

    def script(ctx):
        g = ctx.grads_alloc()
        assert g.d_shs % 16 != 0
        return [frame(ctx, dC, g, deg, log=script.log) for _ in range(2)]
    script.make = lambda **kw: hip_context(sc, cam, T, P, W, H, deg, **kw)
    for det in (True, False):
        both(script, det, bin_path=3)
        carried(script.fills, n, 3 * (deg + 1) ** 2, det)


def test_stale_rows():
    """three frames alternating two cameras on ONE ctx: every frame's gradients equal those of a fresh ctx that renders that frame alone
    (a 2-D gradient row the forward's fill missed would carry the previous camera's sums)"""
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 3000, 160, 120, 2
    views = [scene(n, W, H, deg, 5, 0.5, view=v) for v in (0, 1)]
    sc = views[0][0]
    dC = synthetic.make_dC(W, H, 5)
    order = (0, 1, 0)

    def script(ctx):
        g = ctx.grads_alloc()
        out = []
        for v in order:
            set_cam(ctx, views[v][1], views[v][2], views[v][3], W, H)
            out.append(frame(ctx, dC, g, deg, log=script.log))
        return out
    script.make = lambda **kw: hip_context(sc, views[0][1], views[0][2], views[0][3], W, H, deg, **kw)
    got = both(script, True, bin_path=3)
    carried(script.fills, n, 3 * (deg + 1) ** 2, True)
    alone = {}
    for v in set(order):
        ctx = hip_context(sc, views[v][1], views[v][2], views[v][3], W, H, deg, deterministic=True, bin_path=3)
        alone[v] = frame(ctx, dC, ctx.grads_alloc(), deg)
        ctx.close()
    assert_same(got, [alone[v] for v in order], True, "fresh ctx")
    assert not same_bits(alone[0][2]["shs"], alone[1][2]["shs"])          # the two cameras do differ


def test_poisoned_destination():
    """gradient arrays full of NaN before an overwriting backward: every float is written, the SH rows no pixel touched come back as + 0.0"""
    import torch
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H, deg = 2001, 128, 96, 3
    K3 = 3 * (deg + 1) ** 2
    sc, cam, T, P = scene(n, W, H, deg, 9, 0.7)
    sc["means"][:64, 0] += np.float32(1.0e4)                              # off screen: no pixel touches them
    dC = synthetic.make_dC(W, H, 9)
    outs = []
    for extra in (0, NO_TAIL_FILL):
        ctx = hip_context(sc, cam, T, P, W, H, deg, deterministic=True, bin_path=3, debug_flags=extra)
        frames = []
        for _ in range(2):                                                # the second frame's forward carries the fill of the 2-D rows
            flat = torch.full((n * (11 + K3) + 8,), float("nan"), dtype=torch.float32, device="cuda")
            ptrs, o = [], 0
            for w in (3, 3, 4, 1, K3):
                ptrs.append(flat[o:o + n * w].data_ptr()); o += n * w
            assert ptrs[4] % 16 != 0
            torch.cuda.synchronize()
            ctx.preprocess(); ctx.bin()
            ctx.forward_host()
            ctx.backward(dC, B.GsGrads(*ptrs), overwrite=True); ctx.synchronize()
            assert ctx.tail_fill_blocks() == ((0, 0) if extra else (blocks(n * 128) if frames else 0, blocks(n * K3 * 4)))
            h = flat.cpu().numpy()
            assert np.isnan(h[o:]).all()                                  # nothing written behind the arrays
            frames.append(h[:o].copy())
        outs.append(frames)
        ctx.close()
    for a, b in zip(*outs):
        assert not np.isnan(a).any() and not np.isnan(b).any()
        assert same_bits(a, b)
        shs = a[11 * n:].reshape(n, K3)
        untouched = ~np.any(shs != 0.0, axis=1)
        assert untouched[:64].all() and 64 <= untouched.sum() < n
        assert not bits(shs[untouched]).any()                             # + 0.0: no sign bit
        assert np.any(shs[~untouched] != 0.0, axis=1).all()


@pytest.mark.parametrize("det", [True, False])
def test_call_orders(det):
    from gaussiansplat_amd import synthetic
    n, W, H, deg = 3000, 160, 120, 3
    views = [scene(n, W, H, deg, 13, 0.5, view=v) for v in (0, 1)]
    sc, cam, T, P = views[0]
    dC = synthetic.make_dC(W, H, 13)
    make = lambda **kw: hip_context(sc, cam, T, P, W, H, deg, **kw)

    def fwd_fwd_bwd(ctx):
        g = ctx.grads_alloc()
        out = []
        for _ in range(2):
            ctx.preprocess(); ctx.bin()
            ctx.forward_host()
            img, tr = ctx.forward_host()
            ctx.backward(dC, g, overwrite=True)
            fwd_fwd_bwd.log.append(ctx.tail_fill_blocks())
            out.append((img, tr, ctx.grads_read(g, deg)))
        return out

    def split_phases(ctx):                                                # overwrite in two calls: the per-gaussian kernel writes its own zeros
        g = ctx.grads_alloc()
        out = []
        for _ in range(2):
            ctx.preprocess(); ctx.bin()
            img, tr = ctx.forward_host()
            ctx.backward(dC, g, overwrite=True, phase="composite")
            ctx.backward(dC, g, overwrite=True, phase="params")
            split_phases.log.append(ctx.tail_fill_blocks())
            out.append((img, tr, ctx.grads_read(g, deg)))
        return out

    def overwrite_then_accumulate(ctx):
        g = ctx.grads_alloc()
        out = []
        for _ in range(2):
            for v, ow in ((0, True), (1, False)):
                set_cam(ctx, views[v][1], views[v][2], views[v][3], W, H)
                out.append(frame(ctx, dC, g, deg, overwrite=ow, log=overwrite_then_accumulate.log))
        return out

    def render_only(ctx):
        out = []
        for _ in range(3):
            ctx.preprocess(); ctx.bin()
            out.append(ctx.forward_host() + (None,))
            render_only.log.append(ctx.tail_fill_blocks())
        return out

    ref = None
    for script in (fwd_fwd_bwd, split_phases, overwrite_then_accumulate, render_only):
        script.make = make
        got = both(script, det, bin_path=3)
        if script in (fwd_fwd_bwd, split_phases):                         # the same frame by three call orders
            if ref is None:
                ref = got
            assert_same(got, ref, det, script.__name__ + " against fwd_fwd_bwd")
        if script is render_only:
            assert_same([f[:2] + (None,) for f in ref[:1]], got[:1], det, "render only")
    fwd, bwd = blocks(n * 16 * (8 if det else 4)), blocks(n * 3 * (deg + 1) ** 2 * 4)
    # the frame's second forward finds the rows its first one cleared; split phases keep the per-gaussian kernel's own zeros, and so does an
    # accumulating view; a ctx that never calls backward has no gradient rows to clear
    assert fwd_fwd_bwd.fills == [(0, bwd), (0, bwd)], fwd_fwd_bwd.fills
    assert split_phases.fills == [(0, 0), (fwd, 0)], split_phases.fills
    assert overwrite_then_accumulate.fills == [(0, bwd), (fwd, 0), (fwd, bwd), (fwd, 0)], overwrite_then_accumulate.fills
    assert render_only.fills == [(0, 0)] * 3, render_only.fills


@pytest.mark.parametrize("det", [True, False])
def test_2d_renderer(det):
    """the 2-D renderer: the forward's fill of the 2-D gradient rows only (a ctx's second frame carries it)"""
    from gaussiansplat_amd import backend as B, synthetic
    n, W, H = 777, 90, 70
    sc = synthetic.make_scene_2d(n, W, H, 7, scale_hi=SCALE_HI_2D)
    dC = synthetic.make_dC(W, H, 7)

    def script(ctx):
        g = ctx.grads_alloc()
        out = []
        for _ in range(2):
            ctx.preprocess(); ctx.bin()
            img, tr = ctx.forward_host()
            ctx.backward(dC, g, overwrite=True)
            script.log.append(ctx.tail_fill_blocks())
            out.append((img, tr, ctx.grads_read_2d(g)))
        return out

    def make(**kw):
        ctx = B.Context(order=B.ORDER_INDEX, **kw)
        ctx.set_model_2d_host(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"])
        ctx.set_image_size(W, H)
        return ctx
    script.make = make
    both(script, det, bin_path=3)
    assert script.fills == [(0, 0), (blocks(n * 16 * (8 if det else 4)), 0)], script.fills
