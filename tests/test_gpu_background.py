"""The background colour (gs_set_background / gs_compose_target) on the MI355X.

Forward: bit for bit C + float32(T * bg) of the same build's black-background frame (NumPy float32: one multiply, one add), on every
composite path.  Gradients: the oracle's adjoint on the DC-SHIFTED TWIN (tests/test_background_host.py pins that reference), at the
project's rel-L2 bar of 1e-3; the fused backwards bit for bit against their two-step forms.  Shapes are the smallest that take a path:
561 pixels (scalar kernel and its tail), ragged 200 x 120 (vector kernel), a dense scene whose pixels freeze, depth slabs, four waves
per tile, the 2-D renderer."""
import ctypes as C
import functools

import numpy as np
import pytest

from common import GRADS, hip_context, refused, rel_l2, same_bits, scene_and_cameras

pytestmark = pytest.mark.gpu

BG = (1.0, 0.25, 0.6)
SH_C0 = 0.28209479177387814
PIX_ATOL, PIX_RTOL = 1e-4, 1e-4                                            # tests/test_gpu_parity.py
GRAD_REL_L2 = 1e-3
GRADS_2D = ("means", "scales", "rots", "opacities", "colors")
LR6 = (1e-3, 4e-3, 2e-3, 5e-2, 2.5e-3, 1.25e-4)
B1, B2, EPS = 0.9, 0.999, 1e-8

# name -> (n, W, H, deg, seed, scale boost, ctx keywords)
SCENES = {
    "small": (300, 33, 17, 0, 5, 0.0, dict(t_min=1e-5, tile_parts=1)),
    "ragged_t0": (3001, 200, 120, 1, 7, 0.0, dict(t_min=0.0, tile_parts=1)),
    "ragged_t1e-5": (3001, 200, 120, 1, 7, 0.0, dict(t_min=1e-5, tile_parts=1)),
    "dense": (4000, 80, 56, 2, 17, 1.2, dict(t_min=0.2, tile_parts=1)),
    "dense_t1e-3": (4000, 80, 56, 2, 17, 1.2, dict(t_min=1e-3, tile_parts=1)),
    "slabs": (5000, 112, 72, 2, 17, 1.2, dict(t_min=1e-3, tile_parts=1, slab_mode=1, slab_fractions=(0.15, 0.5))),
    "parts": (3001, 200, 120, 1, 7, 0.0, dict(t_min=1e-5, tile_parts=4)),
}
# (n, W, H, seed, scale_hi) of tests/test_gpu_2d.py: the ragged one.  Its third case (777 gaussians on 90 x 70) is opaque nearly everywhere
# (mean T 1.6e-4): the oracle's black-background gradients are then only 0.02 rel-L2 from the twin's, too close to tell the two apart
SCENE_2D = (1501, 200, 120, 6, 2.0)


def _blend(img, tr, bg=BG):
    """What gs_forward must leave: one float32 multiply, then one float32 add."""
    b = np.asarray(bg, np.float32)
    tb = tr[None].astype(np.float32) * b[:, None, None]
    assert tb.dtype == np.float32
    return img.astype(np.float32) + tb


@functools.lru_cache(maxsize=None)
def _scene(name):
    n, W, H, deg, seed, boost, kw = SCENES[name]
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, seed)
    if boost:
        sc["scales"] = sc["scales"] + np.float32(boost)
    return sc, cam, T, P, ocam


def _ctx3d(name, **more):
    n, W, H, deg, seed, boost, kw = SCENES[name]
    sc, cam, T, P, ocam = _scene(name)
    return hip_context(sc, cam, T, P, W, H, deg, order=1, **{**kw, **more})


def _ctx2d(sc, W, H, **kw):
    from gaussiansplat_amd import backend as B
    ctx = B.Context(order=B.ORDER_INDEX, **kw)
    ctx.set_model_2d_host(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"])
    ctx.set_image_size(W, H)
    return ctx


def _frames(ctx, W, H):
    """One frame read through forward_host(), then one into bound device buffers: [(image, transmittance)] * 2, and what the frames were."""
    import torch
    out = []
    ctx.preprocess(); ctx.bin()
    info = dict(rounds=ctx.num_rounds)
    out.append(ctx.forward_host())
    info["parts"] = ctx.tile_parts_of_frame()
    timg = torch.full((3, H, W), float("nan"), device="cuda")
    ttr = torch.full((H, W), float("nan"), device="cuda")
    torch.cuda.synchronize()
    ctx.bind_outputs(timg.data_ptr(), ttr.data_ptr())
    ctx.preprocess(); ctx.bin()
    ctx.forward_device(timg.data_ptr(), ttr.data_ptr())
    ctx.synchronize()
    out.append((timg.cpu().numpy(), ttr.cpu().numpy()))
    ctx.bind_outputs(0, 0)
    return out, info


# ---------------------------------------------------------------- a. forward, bit for bit against the same build at black
@pytest.mark.parametrize("name", ["small", "ragged_t0", "ragged_t1e-5", "dense", "slabs", "parts", "2d"])
def test_forward_is_the_black_frame_plus_t_times_background(name):
    if name == "2d":
        from gaussiansplat_amd import synthetic
        n, W, H, seed, shi = SCENE_2D
        sc = synthetic.make_scene_2d(n, W, H, seed, scale_hi=shi)
        make = lambda **kw: _ctx2d(sc, W, H, tile_parts=1, **kw)
    else:
        W, H = SCENES[name][1:3]
        make = lambda **kw: _ctx3d(name, **kw)
    black, ctx = make(), make()
    assert ctx.background == (0.0, 0.0, 0.0)
    ctx.set_background(BG)
    assert ctx.background == tuple(float(np.float32(x)) for x in BG)
    want, info0 = _frames(black, W, H)
    got, info = _frames(ctx, W, H)
    assert info == info0
    if name == "slabs":
        assert info["rounds"] == 3                                          # the blend had to follow the last round
    if name == "parts":
        assert info["parts"] == 4
    if name == "dense":                                                     # pixels really froze: the transmittance is not the literal one
        lit = _ctx3d(name, t_min=0.0)
        lit.preprocess(); lit.bin()
        assert not np.array_equal(lit.forward_host()[1], want[0][1])
        lit.close()
    for how, (img, tr), (img0, tr0) in zip(("host", "bound"), got, want):
        assert np.isfinite(img0).all() and tr0.max() > 0.0                 # some pixels are not opaque: the background shows
        assert np.array_equal(tr, tr0), how
        assert np.array_equal(img, _blend(img0, tr0)), (how, np.abs(img - _blend(img0, tr0)).max())
        assert not np.array_equal(img, img0), how
    black.close(); ctx.close()


# ---------------------------------------------------------------- b. forward against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_ref(name):
    from oracle import oracle as O
    O.build()
    n, W, H, deg, seed, boost, kw = SCENES[name]
    sc, cam, T, P, ocam = _scene(name)
    return O.render(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam, order=1, t_min=kw["t_min"])


@pytest.mark.parametrize("name", ["ragged_t0", "ragged_t1e-5"])
def test_forward_pixels_against_the_oracle(oracle, name):
    ref = _oracle_ref(name)
    want = ref["image"].astype(np.float64) + ref["trans"].astype(np.float64)[None] * np.asarray(BG, np.float64)[:, None, None]
    ctx = _ctx3d(name)
    ctx.set_background(BG)
    ctx.preprocess(); ctx.bin()
    img, tr = ctx.forward_host()
    assert np.all(np.abs(img - want) <= PIX_ATOL + PIX_RTOL * np.abs(want)), np.abs(img - want).max()
    assert np.all(np.abs(tr - ref["trans"]) <= PIX_ATOL + PIX_RTOL * np.abs(ref["trans"]))
    ctx.close()


# ---------------------------------------------------------------- c. gradients against the oracle's twin
@pytest.mark.parametrize("name", ["ragged_t0", "ragged_t1e-5", "dense_t1e-3"])
def test_gradients_are_the_oracle_twins(oracle, name):
    from gaussiansplat_amd import synthetic
    O = oracle
    n, W, H, deg, seed, boost, kw = SCENES[name]
    sc, cam, T, P, ocam = _scene(name)
    ref = _oracle_ref(name)
    dC = synthetic.make_dC(W, H, seed)
    twin_shs = sc["shs"].copy()
    twin_shs[:, 0, :] -= (np.asarray(BG, np.float64) / SH_C0).astype(np.float32)
    back = lambda shs: O.backward(sc["means"], sc["scales"], sc["quats"], sc["opacities"], shs, deg, ocam, ref["ranges"], ref["ids"], dC,
                                  t_min=kw["t_min"])
    gref, black = back(twin_shs), back(sc["shs"])
    # a condition on the INPUT: the background moves these gradients far beyond the bar, so ignoring it cannot pass
    assert rel_l2(black["means"].reshape(-1), gref["means"].reshape(-1)) > 0.1
    ctx = _ctx3d(name)
    ctx.set_background(BG)
    ctx.preprocess(); ctx.bin(); ctx.forward_host()
    g = ctx.grads_alloc()
    ctx.backward(dC, g); ctx.backward(dC, g)                              # gradients ACCUMULATE: two calls = 2x
    got = ctx.grads_read(g, deg)
    for k in GRADS:
        err = rel_l2(got[k].reshape(-1).astype(np.float64) / 2.0, gref[k].reshape(-1))
        print(name, k, "rel-L2 against the twin", err, "black against the twin", rel_l2(black[k].reshape(-1), gref[k].reshape(-1)))
        assert err <= GRAD_REL_L2, (k, err)
    ctx.close()


@pytest.mark.parametrize("t_min", [0.0, 1e-5])
def test_gradients_2d_are_the_oracle_twins(oracle, t_min):
    from gaussiansplat_amd import synthetic
    O = oracle
    n, W, H, seed, shi = SCENE_2D
    sc = synthetic.make_scene_2d(n, W, H, seed, scale_hi=shi)
    ref = O.render2d(sc["means"], sc["scales"], sc["rots"], sc["opacities"], sc["colors"], W, H, t_min=t_min)
    dC = synthetic.make_dC(W, H, seed)
    twin = (sc["colors"] - np.asarray(BG, np.float32)[None]).astype(np.float32)      # the 2-D colours are used raw: the twin is colors - bg
    back = lambda colors: O.backward2d(sc["means"], sc["scales"], sc["rots"], sc["opacities"], colors, W, H, ref["ranges"], ref["ids"], dC,
                                       t_min=t_min)
    gref, black = back(twin), back(sc["colors"])
    assert rel_l2(black["means"].reshape(-1), gref["means"].reshape(-1)) > 0.1
    ctx = _ctx2d(sc, W, H, t_min=t_min)
    ctx.set_background(BG)
    ctx.preprocess(); ctx.bin()
    img, tr = ctx.forward_host()
    want = ref["image"].astype(np.float64) + ref["trans"].astype(np.float64)[None] * np.asarray(BG, np.float64)[:, None, None]
    assert np.all(np.abs(img - want) <= PIX_ATOL + PIX_RTOL * np.abs(want))
    g = ctx.grads_alloc()
    ctx.backward(dC, g); ctx.backward(dC, g)
    got = ctx.grads_read_2d(g)
    for k in GRADS_2D:
        err = rel_l2(got[k].reshape(-1).astype(np.float64) / 2.0, gref[k].reshape(-1))
        print("2d", t_min, k, "rel-L2 against the twin", err)
        assert err <= GRAD_REL_L2, (k, err)
    ctx.close()


# ---------------------------------------------------------------- d. fused forms
FN, FW, FH, FDEG = 1281, 128, 96, 1


class _Rig:
    """One deterministic ctx over a device copy of a scene, on the legacy default stream (in order with torch's copies)."""

    def __init__(self, sc, deg, w, h, bg=None):
        import torch
        from gaussiansplat_amd import backend as B
        self.n, self.deg, self.w, self.h = sc["means"].shape[0], deg, w, h
        self.ctx = B.Context(deterministic=True, tile_parts=1)
        self.ctx.set_stream(1)
        self.p = [torch.as_tensor(np.ascontiguousarray(sc[k], np.float32).reshape(self.n, -1)).cuda().contiguous() for k in GRADS]
        self.ctx.set_model_device(self.n, deg, [t.data_ptr() for t in self.p])
        if bg is not None:
            self.ctx.set_background(bg)

    def frame(self, v=0):
        from gaussiansplat_amd import camera as gcam, synthetic
        cam = synthetic.scene_camera(self.w, view=v)
        f = lambda x: float(np.float32(x))
        self.ctx.set_camera(gcam.compute_transform(cam), gcam.compute_projection(cam, self.w, self.h), f(cam.fx), f(cam.fy), f(cam.near),
                            f(cam.far), cam.eye, cam.lookAt, self.w, self.h)
        self.ctx.preprocess(); self.ctx.bin()
        self.ctx.forward_device(0, 0)

    def close(self):
        self.ctx.close()

    def buffers(self, fill):
        """five device arrays of the model's widths (views into one flat buffer) and their gs_grads"""
        import torch
        from gaussiansplat_amd import backend as B
        widths = [3, 3, 4, 1, 3 * (self.deg + 1) ** 2]
        flat = torch.empty(sum(widths) * self.n, device="cuda")
        ts, o = [], 0
        for i, w in enumerate(widths):
            ts.append(flat[o:o + w * self.n].view(self.n, w)); o += w * self.n
            ts[-1].copy_(torch.as_tensor(fill(i, (self.n, w))))
        return ts, B.GsGrads(*[t.data_ptr() for t in ts])


def _fused_scene():
    from gaussiansplat_amd import synthetic
    return synthetic.make_scene(FN, FW, FH, FDEG, seed=231)


def _device_dC(w, h, seed):
    import torch
    from gaussiansplat_amd import synthetic
    return torch.as_tensor(synthetic.make_dC(w, h, seed)).cuda()


@pytest.mark.parametrize("selective", [False, True], ids=["dense", "selective"])
def test_backward_adam_equals_backward_then_adam_step_under_a_background(selective):
    import torch
    sc, dC = _fused_scene(), _device_dC(FW, FH, 902)
    rng = np.random.default_rng(41)
    widths = (3, 3, 4, 1, 3 * (FDEG + 1) ** 2)
    m0 = [(0.01 * rng.standard_normal((FN, w))).astype(np.float32) for w in widths]
    v0 = [(0.01 * rng.random((FN, w)) + 1e-6).astype(np.float32) for w in widths]
    res = {}
    for how, bg in (("fused", BG), ("steps", BG), ("black", None)):
        rig = _Rig(sc, FDEG, FW, FH, bg)
        (mt, m), (vt, v) = rig.buffers(lambda i, s: m0[i]), rig.buffers(lambda i, s: v0[i])
        rig.frame(0)
        if how == "steps":
            gt, g = rig.buffers(lambda i, s: np.full(s, np.nan, np.float32))
            rig.ctx.backward(dC.data_ptr(), g, overwrite=True)
            rig.ctx.adam_step(g, m, v, LR6, B1, B2, EPS, 3, selective=selective)
        else:
            rig.ctx.backward_adam(dC.data_ptr(), m, v, LR6, B1, B2, EPS, 3, selective=selective)
        torch.cuda.synchronize()
        res[how] = [t.cpu().numpy().copy() for t in rig.p + mt + vt]
        rig.close()
    for k, (a, b) in enumerate(zip(res["fused"], res["steps"])):
        assert same_bits(a, b), k
    assert not same_bits(res["fused"][0], res["black"][0])                      # the background reached the step of the means


def test_backward_sgd_equals_backward_then_sgd_step_under_a_background():
    import torch
    sc, dC = _fused_scene(), _device_dC(FW, FH, 903)
    res = {}
    for how, bg in (("fused", BG), ("steps", BG), ("black", None)):
        rig = _Rig(sc, FDEG, FW, FH, bg)
        rig.frame(0)
        if how == "steps":
            gt, g = rig.buffers(lambda i, s: np.full(s, np.nan, np.float32))
            rig.ctx.backward(dC.data_ptr(), g, overwrite=True)
            rig.ctx.sgd_step(0.05, g)
        else:
            rig.ctx.backward_sgd(dC.data_ptr(), 0.05)
        torch.cuda.synchronize()
        res[how] = [t.cpu().numpy().copy() for t in rig.p]
        rig.close()
    for k, (a, b) in enumerate(zip(res["fused"], res["steps"])):
        assert same_bits(a, b), k
    assert not same_bits(res["fused"][0], res["black"][0])


# ---------------------------------------------------------------- e. contract
def test_contract_default_refusals_and_the_frame():
    from gaussiansplat_amd import backend as B
    ctx = _ctx3d("small")
    L, h = ctx.L, ctx.h
    assert ctx.background == (0.0, 0.0, 0.0)
    ctx.set_background((0.5, 0.25, 0.125))
    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))):
        assert L.gs_set_background(h, (C.c_float * 3)(*bad)) == B.GS_ERR_INVALID
        assert ctx.background == (0.5, 0.25, 0.125)                       # a refused call changes nothing
    with pytest.raises(ValueError):
        ctx.set_background((1.0, 2.0))
    n, W, H, deg = SCENES["small"][:4]
    dC = np.ones((3, H, W), np.float32)
    g = ctx.grads_alloc()
    ctx.preprocess(); ctx.bin(); ctx.forward_host()
    ctx.backward(dC, g)
    ctx.set_background((0.5, 0.25, 0.125))                                # the value in force: the frame stands
    ctx.backward(dC, g)
    ctx.set_background(BG)                                                # a changed value: the image is stale ...
    refused(lambda: ctx.backward(dC, g), "gs_forward first")
    img, tr = ctx.forward_host()                                          # ... the lists are not: no gs_bin needed
    ctx.backward(dC, g)
    black = _ctx3d("small")
    black.preprocess(); black.bin()
    img0, tr0 = black.forward_host()
    assert np.array_equal(img, _blend(img0, tr0)) and np.array_equal(tr, tr0)
    # (0, 0, 0) set explicitly renders what a ctx that never heard of backgrounds renders
    ctx.set_background((0.0, 0.0, 0.0))
    ctx.preprocess(); ctx.bin()
    img, tr = ctx.forward_host()
    assert np.array_equal(img, img0) and np.array_equal(tr, tr0)
    ctx.close(); black.close()


def test_contract_the_request_survives_set_model():
    ctx = _ctx3d("small")
    ctx.set_background(BG)
    n, W, H, deg = SCENES["ragged_t0"][:4]
    sc, cam, T, P, ocam = _scene("ragged_t0")                              # another size and another degree
    ctx.set_model_host(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"].reshape(n, -1), deg)
    assert ctx.background == tuple(float(np.float32(x)) for x in BG)
    ctx.set_camera(T, P, float(np.float32(cam.fx)), float(np.float32(cam.fy)), float(np.float32(cam.near)), float(np.float32(cam.far)),
                   cam.eye, cam.lookAt, W, H)
    ctx.preprocess(); ctx.bin()
    img, tr = ctx.forward_host()
    black = _ctx3d("ragged_t0", t_min=1e-5)                                # (the first ctx was made with the small scene's t_min)
    black.preprocess(); black.bin()
    img0, tr0 = black.forward_host()
    assert np.array_equal(img, _blend(img0, tr0)) and np.array_equal(tr, tr0)
    ctx.close(); black.close()


def test_contract_the_request_survives_a_density_restructure():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.density import DensityController
    from gaussiansplat_amd.optim import Adam
    sc = synthetic.make_scene(FN, FW, FH, 2, seed=184)
    cam = synthetic.scene_camera(FW)
    r = R.getRenderer("GAUSSIAN_3D", (FW, FH, 3), (16, 16), None, sc, deterministic=True, tile_parts=1, background=BG)
    want = tuple(float(np.float32(x)) for x in BG)
    assert r.background == want
    lf = TR.getLossFunction((FW, FH, 3), 11, 3, renderer=r)
    gt = torch.rand((3, FH, FW), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    extent = float(np.linalg.norm(sc["means"].max(0) - sc["means"].min(0)) / 2)
    ctl = DensityController(scene_extent=extent, from_iter=1, until_iter=10, interval=2, opacity_reset_interval=0, grad_threshold=2e-6,
                            generator=torch.Generator("cuda").manual_seed(6))
    opt = Adam(r, lr=1e-3)
    for _ in range(2):
        TR.trainStep(r, gt, 0.0, lf, cam, want_loss=False, optimizer=opt, density=ctl)
    assert len(ctl.history) == 1 and r.nGaussians != FN                   # one restructure: gs_set_model onto a model of another size
    assert r.background == want
    tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
    img, tr = r.imageData.clone(), r.transmittance.clone()
    r.background = (0.0, 0.0, 0.0)
    R.forward(r, tps)                                                      # the lists stand
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), _blend(r.imageData.cpu().numpy(), r.transmittance.cpu().numpy()))
    assert torch.equal(tr, r.transmittance)


def test_contract_debug_launches_leave_the_blended_image():
    import torch
    W, H = SCENES["ragged_t1e-5"][1:3]
    ctx = _ctx3d("ragged_t1e-5")
    ctx.set_background(BG)
    timg, ttr = torch.zeros((3, H, W), device="cuda"), torch.zeros((H, W), device="cuda")
    torch.cuda.synchronize()
    ctx.bind_outputs(timg.data_ptr(), ttr.data_ptr())
    ctx.preprocess(); ctx.bin()
    ctx.forward_device(timg.data_ptr(), ttr.data_ptr())
    ctx.synchronize()
    img, tr = timg.cpu().numpy(), ttr.cpu().numpy()
    black = _ctx3d("ragged_t1e-5")
    black.preprocess(); black.bin()
    img0, tr0 = black.forward_host()
    assert np.array_equal(img, _blend(img0, tr0)) and not np.array_equal(img, img0)
    assert ctx.time_composite(0, 0, reps=1) >= 0.0                         # re-launches the forward into the bound image ...
    ctx.synchronize()
    assert np.array_equal(timg.cpu().numpy(), img) and np.array_equal(ttr.cpu().numpy(), tr)      # ... which stays what gs_forward left
    ctx.tile_clock(0, 10)
    ctx.synchronize()
    assert np.array_equal(timg.cpu().numpy(), img) and np.array_equal(ttr.cpu().numpy(), tr)
    ctx.close(); black.close()


# ---------------------------------------------------------------- f. gs_compose_target
@pytest.mark.parametrize("W,H,offset", [(33, 17, 0), (200, 120, 0), (200, 120, 1)], ids=["33x17", "200x120", "200x120-unaligned"])
def test_compose_target_is_the_four_operation_formula(W, H, offset):
    """offset: floats the base pointers are shifted by -- a plane length that is a multiple of four on bases that are not 16-byte aligned
    takes the scalar kernel, and must give the same values."""
    import torch
    from gaussiansplat_amd import backend as B
    rng = np.random.default_rng(W + offset)
    rgba = rng.random((4, H, W), dtype=np.float32)
    a = rgba[3]
    pick = rng.random((H, W))
    a[pick < 0.2] = 0.0
    a[pick > 0.8] = 1.0
    assert (a == 0).any() and (a == 1).any() and ((a > 0) & (a < 1)).any()
    px = W * H
    src = torch.zeros(4 * px + 4, device="cuda")
    dst = torch.full((3 * px + 4,), float("nan"), device="cuda")
    src[offset:offset + 4 * px].copy_(torch.as_tensor(rgba.reshape(-1)))
    ctx = B.Context()
    ctx.set_stream(1)
    ctx.set_background(BG)
    sp, dp = src.data_ptr() + 4 * offset, dst.data_ptr() + 4 * offset
    assert (sp % 16 == 0) == (offset == 0)
    ctx.compose_target(sp, W, H, dp)
    torch.cuda.synchronize()
    out = dst[offset:offset + 3 * px].cpu().numpy().reshape(3, H, W)
    bg = np.asarray(BG, np.float32)
    ca = rgba[:3] * a[None]                                                 # four float32 operations, each rounded on its own
    na = np.float32(1.0) - a
    bn = bg[:, None, None] * na[None]
    want = ca + bn
    assert want.dtype == np.float32
    assert np.array_equal(out, want), np.abs(out - want).max()
    assert np.array_equal(out[:, a == 1], rgba[:3][:, a == 1])             # opaque: the target's own colour, exactly
    assert np.array_equal(out[:, a == 0], np.broadcast_to(bg[:, None], out[:, a == 0].shape))    # transparent: the background, exactly
    tail = dst.cpu().numpy()
    assert np.isnan(tail[:offset]).all() and np.isnan(tail[offset + 3 * px:]).all()              # nothing written outside the three planes
    assert ctx.L.gs_compose_target(ctx.h, C.c_void_p(sp), W, H, C.c_void_p(sp + 4 * px)) == B.GS_ERR_INVALID     # overlapping buffers
    assert ctx.L.gs_compose_target(ctx.h, C.c_void_p(sp), 0, H, C.c_void_p(dp)) == B.GS_ERR_INVALID
    ctx.close()


# ---------------------------------------------------------------- g. training
def _rgba_target(W, H, seed):
    import torch
    g = torch.Generator("cuda").manual_seed(seed)
    rgba = torch.rand((4, H, W), device="cuda", generator=g)
    pick = torch.rand((H, W), device="cuda", generator=g)
    rgba[3][pick < 0.3] = 0.0
    rgba[3][pick > 0.7] = 1.0
    return rgba


@pytest.mark.parametrize("how_opt", ["sgd", "fused_adam"])
def test_random_background_equals_a_hand_written_loop(how_opt):
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    from gaussiansplat_amd.optim import Adam
    W, H, n, deg = 64, 48, 500, 1
    sc = synthetic.make_scene(n, W, H, deg, seed=290)
    cam = synthetic.scene_camera(W)
    rgba = _rgba_target(W, H, 9)
    snaps = {}
    for how in ("train_step", "by_hand", "black"):
        r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
        R.resetGrads(r)
        lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
        opt = Adam(r, lr=1e-3, fused=True) if how_opt == "fused_adam" else None
        bg, rng = TR.RandomBackground(3), np.random.default_rng(3)
        target = torch.empty((3, H, W), device="cuda")
        for it in range(3):
            if how == "train_step":
                TR.trainStep(r, rgba, 0.05, lf, cam, want_loss=False, optimizer=opt, background=bg)
                assert bg.iteration == it + 1
            else:
                rgb = rng.random(3, dtype=np.float32)                       # the same generator, the same draws
                r.background = (0.0, 0.0, 0.0) if how == "black" else tuple(float(x) for x in rgb)
                r._begin()
                r.ctx.compose_target(rgba.data_ptr(), W, H, target.data_ptr())
                tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
                _, dC = lf.value_and_grad(r.imageData, target, False)
                if opt is not None:
                    opt.backward_step(dC)
                else:
                    R.backward(r, dC)
                    r._begin()
                    r.ctx.sgd_step(0.05, r._grads)
                    R.resetGrads(r)
            if how != "black":
                assert r.background == tuple(float(x) for x in np.random.default_rng(3).random((it + 1, 3), dtype=np.float32)[it])
        torch.cuda.synchronize()
        sd = r.splatData
        snaps[how] = [t.clone() for t in (sd.means, sd.scales, sd.quaternions, sd.opacities, sd.shs)]
    for k, (a, b) in enumerate(zip(snaps["train_step"], snaps["by_hand"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert not torch.equal(snaps["train_step"][0], snaps["black"][0])     # the colours drawn did reach the parameters


def test_train_step_sets_a_fixed_background_and_takes_a_plain_target():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    W, H, n, deg = 64, 48, 500, 1
    sc = synthetic.make_scene(n, W, H, deg, seed=291)
    cam = synthetic.scene_camera(W)
    rgba = _rgba_target(W, H, 10)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    TR.trainStep(r, rgba[:3].contiguous(), 0.05, lf, cam, want_loss=False, background=(0.5, 0.5, 1.0))
    assert r.background == (0.5, 0.5, 1.0)
    TR.trainStep(r, rgba, 0.05, lf, cam, want_loss=False)                  # None: the renderer's background stays, the RGBA target follows it
    assert r.background == (0.5, 0.5, 1.0)
    torch.cuda.synchronize()
    a = rgba[3]
    want = rgba[:3] * a + torch.tensor([0.5, 0.5, 1.0], device="cuda")[:, None, None] * (1.0 - a)
    assert torch.equal(lf._target, want)


def test_pipelined_view_batch_follows_the_renderers_background():
    """distributed.multi_view_step renders a rank's views on twin renderers with ctxs of their own: they take the background of the rank's
    renderer, also when it changes between two batches; the batch equals the views rendered one after the other."""
    import torch
    from gaussiansplat_amd import distributed as D, renderer as R, synthetic
    sc = synthetic.make_scene(FN, FW, FH, 1, seed=200)
    cams = [synthetic.scene_camera(FW, view=v) for v in range(3)]
    dCs = [_device_dC(FW, FH, 910 + v) for v in range(3)]
    r = R.getRenderer("GAUSSIAN_3D", (FW, FH, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    r2 = R.getRenderer("GAUSSIAN_3D", (FW, FH, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    hv = D.HipViewRenderer(r)
    flats = []
    for bg in (BG, (0.0, 0.0, 0.0), (0.1, 0.9, 0.3)):
        r.background = r2.background = bg
        R.resetGrads(r)
        flat = D.multi_view_step(hv, cams, dCs, exchange=False).clone()
        R.resetGrads(r2)
        for cam, dC in zip(cams, dCs):
            R.forward(r2, (R.preprocess(r2, cam), R.compactIdxs(r2))[0])
            R.backward(r2, dC)
        torch.cuda.synchronize()
        assert torch.equal(flat.view(torch.int32), r2.splatGrads.flat.view(torch.int32)), bg
        flats.append(flat)
    assert not torch.equal(flats[0][:3 * FN], flats[1][:3 * FN]) and not torch.equal(flats[2][:3 * FN], flats[1][:3 * FN])
