"""The camera gradient on the device (gs_backward_camera; renderer.backwardCamera, train(..., pose=...)).

1. consistency with the gradients the project already trusts: the reference camera has orthonormal rows and a zero fourth row, so
   dt[0:3] = R_cam d_means_g and d_T[i + 4 j] = sum_g (R_cam d_means_g)[i] mh_g[j] for i < 3 -- the right-hand side in float64 from the
   device's own d_means (an overwriting gs_backward on the same frame).  Bound per component: 2^-22 x sum_g |term_g| -- one fp32 rounding
   of each d_means entry, one of R_cam, one of the final cast, and a factor two.  Derived, not fitted.  Beside it the covariance path is
   pinned to the device's own d_scales: fx d_fx + fy d_fy = sum d_scales (_scale_relation).
2. end to end against the fp64 adjoint (tests/camera_ref.py through torch_ref.composite on the oracle's lists): per array
   || got - ref || <= 1e-3 || S ||, S_c = sum_g |contribution_{g, c}| (DESIGN.md 2.1's bar, on the absolute mass: these sums cancel).
   Its teeth are checked on the CPU (tests/test_camera_grad_host.py).
3. shapes where the reduction can go wrong (identity 1): N = 1, 63, 65, 257, 256 * 257 + 1; N = 0
4. purity: the same 160 bytes call to call, ctx to ctx, HOST and DEVICE; the frame untouched (a twin ctx that never made the call)
5. refusals, after which the frame goes on
6. planted gaussians (mean at the eye, NaN mean, scale 200) in a live scene
7. an active degree below the stored one; a background colour
8. it descends: a frozen model, the eye displaced by 1 %, train(..., pose=CameraAdam(...), freeze_model=True)"""
import dataclasses

import numpy as np
import pytest
import torch

import camera_ref
from common import hip_context, on_torch_stream, refused, run_frame, same_bits, scene_and_cameras
from gaussiansplat_amd import synthetic

pytestmark = pytest.mark.gpu


def _ctx(sc, cam, T, P, W, H, deg, **kw):
    return on_torch_stream(hip_context(sc, cam, T, P, W, H, deg, **kw))


def _frame(ctx, dC, deg):
    """preprocess .. backward (overwriting): the frame gs_backward_camera follows"""
    return run_frame(ctx, dC, deg, overwrite=True)


def _identity(got40, d_means, means, T, keep=None):
    """|d_T[i + 4 j] - sum_g term_g| <= 2^-22 sum_g |term_g|, term_g = (R_cam d_means_g)[i] mh_g[j], i < 3: the issue's bound, asserted in
    every case.  (Printed beside it, for information: the ratio to the wider mass of the elementary products R[i, k] d_means_g[k] mh_g[j].)
    The right-hand side carries the fp32 rounding of the device's own d_means: where R d_means cancels -- along the view axis, i = 2,
    for a gaussian near the optical axis, whose image hardly moves with its depth -- that rounding alone can exceed 2^-22 |term|.  A sum
    over many gaussians averages it out; the single gaussian of test 3 is therefore placed off the axis (see there)."""
    R = np.asarray(T, np.float32).astype(np.float64).reshape(4, 4, order="F")[:3, :3]
    dm, m = np.asarray(d_means, np.float64), np.asarray(means, np.float64)
    if keep is not None:
        dm, m = dm[keep], m[keep]
    mh = np.concatenate([m, np.ones((m.shape[0], 1))], 1)
    prod = R[None, :, :, None] * dm[:, None, :, None] * mh[:, None, None, :]        # [g, i, k, j]
    terms = prod.sum(axis=2)                                                         # (R d_means_g)[i] mh_g[j]
    rhs, mass = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    wide = np.abs(prod).sum(axis=(0, 2))
    got = np.asarray(got40, np.float64)[:16].reshape(4, 4, order="F")[:3, :]
    err, bound = np.abs(got - rhs), 2.0 ** -22 * mass
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if mass.any() else 0.0
    print("identity: worst |got - rhs| / bound =", ratio, " (on the mass of the elementary products:", float((err / np.maximum(2.0 ** -22 * wide, 1e-300)).max()), ")")
    assert (err <= bound).all(), (err, bound)
    return ratio, rhs


def _scale_relation(got40, d_scales, cam):
    """fx d_fx + fy d_fy = sum_g sum_j d_scales[g, j], exactly: J = diag(fx, fy) J0, so scaling fx and fy by (1 + e) scales cov - 0.3 by
    (1 + 2 e), and so does scaling every exp(scale) by (1 + e); neither reaches anything else (P is an input of its own).  It pins the
    covariance path of the camera kernel to the device's own scale gradients whatever the resolution of the rows.
    Bound: 2^-22 x sum |d_scales| -- one fp32 rounding of each d_scales entry, one each of the casts of d_fx and d_fy, a factor two."""
    ds = np.asarray(d_scales, np.float64)
    lhs = float(np.float32(cam.fx)) * float(got40[38]) + float(np.float32(cam.fy)) * float(got40[39])
    rhs, mass = ds.sum(), np.abs(ds).sum()
    print("scale relation: |fx d_fx + fy d_fy - sum d_scales| / bound =", abs(lhs - rhs) / max(2.0 ** -22 * mass, 1e-300))
    assert mass > 0 and abs(lhs - rhs) <= 2.0 ** -22 * mass, (lhs, rhs, mass)


# ---------------------------------------------------------------- 1. consistency with d_means

@pytest.mark.parametrize("deg", [1, 3])
@pytest.mark.parametrize("det", [False, True], ids=["float_atomics", "deterministic"])
def test_d_T_is_the_outer_product_sum_of_the_device_d_means(deg, det):
    n, W, H = 2000, 128, 96
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 500 + deg)
    ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=det, t_min=1e-5)
    g = _frame(ctx, synthetic.make_dC(W, H, 500 + deg), deg)["g"]
    got = ctx.backward_camera()
    assert got.shape == (40,) and got.dtype == np.float32 and np.isfinite(got).all()
    gr = ctx.grads_read(g, deg)
    dm = gr["means"]
    assert np.count_nonzero(dm.any(axis=1)) > n // 10
    _identity(got, dm, sc["means"], T)
    _scale_relation(got, gr["scales"], cam)
    assert got[[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]].any()                     # the twelve values are not all zero
    assert got[16:32].any() and got[38] != 0 and got[39] != 0 and got[32:38].any()


# ---------------------------------------------------------------- 2. end to end against the fp64 adjoint

def test_end_to_end_against_the_fp64_adjoint(oracle):
    """Measured on MI355X, || got - ref || / || S || per array against the bar of 1e-3: d_T 4.4e-6, d_P 2.2e-6, d_eye = d_lookAt 9.0e-7,
    (d_fx, d_fy) 9.7e-4.  The last one is the resolution of the deterministic mode's rows, not the camera kernel: fx and fy see the covariance
    path alone, i.e. the second-order moments, which deterministic mode keeps in 2^-28 fixed point, and this dC = 2 (image - target) / numel
    is of the order of 1e-5.  With float atomics the same case measures 2.2e-6, with dC x 1024 in deterministic mode 5.5e-6, and
    fx d_fx + fy d_fy equals the sum of the device's own d_scales to 1e-8 relative in every mode."""
    s = camera_ref.e2e_setup(oracle)
    n, W, H, deg, cam = s["n"], s["W"], s["H"], s["deg"], s["cam"]
    tgt = _ctx(s["sc"], s["cam2"], s["T2"], s["P2"], W, H, deg, deterministic=True, t_min=0.0)
    tgt.preprocess(); tgt.bin()
    target, _ = tgt.forward_host()
    ctx = _ctx(s["sc"], cam, s["T"], s["P"], W, H, deg, deterministic=True, t_min=0.0)
    ctx.preprocess(); ctx.bin()
    img, _ = ctx.forward_host()
    assert np.abs(img - s["ref"]["image"]).max() < 1e-3 and np.abs(img - target).max() > 1e-2      # the oracle's frame; a target that differs
    dC = camera_ref.mse_dC(img, target)
    g = ctx.grads_alloc()
    ctx.backward(dC, g, overwrite=True)
    got = ctx.backward_camera().astype(np.float64)
    _scale_relation(got, ctx.grads_read(g, deg)["scales"], cam)                     # the kernel's covariance path, whatever the rows resolve
    c = camera_ref.e2e_contributions(s, dC)
    ref, S = c.sum(axis=0), np.abs(c).sum(axis=0)
    ratios = {}
    for name, sl in (("d_T", slice(0, 16)), ("d_P", slice(16, 32)), ("d_f", slice(38, 40)), ("d_eye", slice(32, 35)), ("d_lookAt", slice(35, 38))):
        ratios[name] = float(np.linalg.norm(got[sl] - ref[sl]) / np.linalg.norm(S[sl]))
    print("end to end, || got - ref || / || S ||:", ratios)
    print("end to end, || ref || / || S ||:", {k: float(np.linalg.norm(ref[sl]) / np.linalg.norm(S[sl])) for k, sl in
                                                 (("d_T", slice(0, 16)), ("d_P", slice(16, 32)), ("d_f", slice(38, 40)), ("d_eye", slice(32, 35)))})
    for name, r in ratios.items():
        assert r <= 1e-3, (name, r)


# ---------------------------------------------------------------- 3. shapes where the reduction can go wrong

@pytest.mark.parametrize("n", [1, 63, 65, 257, 256 * 257 + 1])
def test_reduction_shapes(n):
    deg = 1
    W, H = (64, 64) if n > 1000 else (64, 48)
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 600 + n % 97)
    if n == 1:
        # One gaussian, inside the frame and OFF the optical axis, at tx / tz = 0.27, ty = 0: through mu = fx tx / tz its depth adjoint is
        # dt[2] = -(tx / tz) dt[0], a quarter of the lateral one, so R d_means does not cancel on the view-axis row and the fp32 rounding of
        # d_means (2^-24 of |R[2, k] d_means[k]|: 0.03 |dt[0]| + 0.1 |dt[1]| + |dt[2]| for this camera) stays inside 2^-22 |dt[2]|.  On the
        # axis tx / tz is ~ 0 and that rounding alone is several times the bound (measured 3.2 x at (0.5, -0.25, 1)).
        sc["means"][0] = (8.0, 0.0, 0.0)
        sc["scales"][0] = -1.0
    ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=True, t_min=1e-5, slab_mode=0 if n > 1000 else 1)
    g = _frame(ctx, synthetic.make_dC(W, H, 600), deg)["g"]
    assert ctx.num_rounds == 1                                                    # what the case ran: one binning round
    got = ctx.backward_camera()
    dm = ctx.grads_read(g, deg)["means"]
    assert dm.any() and np.isfinite(got).all()
    _identity(got, dm, sc["means"], T)
    assert got[:16].any()


def test_no_gaussians_gives_forty_plus_zeros():
    W, H, deg = 64, 48, 1
    sc, cam, T, P, _ = scene_and_cameras(4, W, H, deg, 7)
    sc = {k: v[:0] for k, v in sc.items()}
    ctx = _ctx(sc, cam, T, P, W, H, deg)
    _frame(ctx, synthetic.make_dC(W, H, 7), deg)
    got = ctx.backward_camera()
    assert got.shape == (40,) and not got.view(np.uint32).any()
    out = torch.full((40,), 7.0, dtype=torch.float32, device="cuda")
    ctx.backward_camera(out.data_ptr())
    torch.cuda.synchronize()
    assert not out.cpu().numpy().view(np.uint32).any()


# ---------------------------------------------------------------- 4. purity

@pytest.mark.parametrize("det", [False, True], ids=["float_atomics", "deterministic"])
def test_two_calls_and_both_memory_kinds_give_the_same_bytes(det):
    n, W, H, deg = 2000, 128, 96, 2
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 700)
    ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=det)
    _frame(ctx, synthetic.make_dC(W, H, 700), deg)
    a, b = ctx.backward_camera(), ctx.backward_camera()
    out = torch.full((40,), 7.0, dtype=torch.float32, device="cuda")
    ctx.backward_camera(out.data_ptr())
    torch.cuda.synchronize()
    assert a.any() and a.nbytes == 160 and same_bits(a, b) and same_bits(a, out)


def _twin_run(sc, cam, T, P, W, H, deg, dC, with_camera):
    from gaussiansplat_amd import backend as B
    ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=True)
    img_t = torch.zeros((3, H, W), dtype=torch.float32, device="cuda"); tr_t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    ctx.bind_outputs(img_t.data_ptr(), tr_t.data_ptr())
    ctx.preprocess(); ctx.bin()
    ctx.forward_device(img_t.data_ptr(), tr_t.data_ptr())
    g = ctx.grads_alloc()
    ctx.backward(dC, g, overwrite=True, phase="composite")
    cg = ctx.backward_camera() if with_camera else None                            # succeeds after GS_BWD_COMPOSITE_ONLY alone
    torch.cuda.synchronize()
    res = dict(img=img_t.cpu().numpy(), tr=tr_t.cpu().numpy(), g2d=ctx.get_array(B.ARR_GRAD2D), work=ctx.work_counters_ex())
    ctx.backward(dC, g, overwrite=True, phase="params")
    res["grads"] = ctx.grads_read(g, deg)
    return res, cg, ctx


def test_the_frame_is_untouched_and_fresh_contexts_agree():
    n, W, H, deg = 2000, 128, 96, 3
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 710)
    dC = synthetic.make_dC(W, H, 710)
    a, cg_a, _ = _twin_run(sc, cam, T, P, W, H, deg, dC, True)
    b, _, _ = _twin_run(sc, cam, T, P, W, H, deg, dC, False)
    c, cg_c, _ = _twin_run(sc, cam, T, P, W, H, deg, dC, True)
    assert cg_a.any() and same_bits(cg_a, cg_c)                                     # deterministic mode: two fresh contexts, the same bytes
    assert a["g2d"].any() and a["img"].any()
    for k in ("img", "tr", "g2d"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert a["work"] == b["work"]
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k].view(np.uint32), b["grads"][k].view(np.uint32)), k


# ---------------------------------------------------------------- 5. refusals

def test_refusals_leave_the_frame_usable():
    from gaussiansplat_amd import backend as B
    n, W, H, deg = 500, 64, 48, 1
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 720)
    dC = synthetic.make_dC(W, H, 720)
    INVALID, UNSUPPORTED = -1, -5
    ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=True)
    refused(ctx.backward_camera, "gs_backward first", INVALID)                     # no frame at all
    ctx.preprocess(); ctx.bin()
    refused(ctx.backward_camera, "gs_backward first", INVALID)                     # before gs_forward
    img, tr = ctx.forward_host()
    refused(ctx.backward_camera, "gs_backward first", INVALID)                     # after gs_forward without a backward
    g = ctx.grads_alloc()
    ctx.backward(dC, g, overwrite=True, phase="composite")
    refused(lambda: ctx.backward_camera(0), "NULL argument", INVALID)              # out == NULL
    got = ctx.backward_camera()                                                     # ... and after GS_BWD_COMPOSITE_ONLY alone it succeeds
    ctx.backward(dC, g, overwrite=True, phase="params")
    grads = ctx.grads_read(g, deg)
    twin = _ctx(sc, cam, T, P, W, H, deg, deterministic=True)                      # the same frame without a refused call in it
    f2 = _frame(twin, dC, deg)
    assert np.array_equal(img, f2["img"]) and np.array_equal(tr, f2["tr"]) and same_bits(got, twin.backward_camera()) and got.any()
    want = twin.grads_read(f2["g"], deg)
    for k in grads:
        assert np.array_equal(grads[k].view(np.uint32), want[k].view(np.uint32)), k
    # after gs_backward_sgd the frame is gone: the stage check refuses; the next frame is served
    ctx.preprocess(); ctx.bin(); ctx.forward_host()
    d = torch.as_tensor(dC).cuda()
    ctx.backward_sgd(d.data_ptr(), 1e-4)
    refused(ctx.backward_camera, "gs_backward first", INVALID)
    _frame(ctx, dC, deg)
    assert np.isfinite(ctx.backward_camera()).all()
    # the 2-D renderer has no camera
    s2 = synthetic.make_scene_2d(200, W, H, seed=3)
    c2 = on_torch_stream(B.Context(deterministic=True))
    c2.set_model_2d_host(s2["means"], s2["scales"], s2["rots"], s2["opacities"], s2["colors"])
    c2.set_image_size(W, H)
    c2.preprocess(); c2.bin()
    i2, _ = c2.forward_host()
    g2d = c2.grads_alloc()
    c2.backward(dC, g2d, overwrite=True)
    refused(c2.backward_camera, "3-D renderer only", UNSUPPORTED)
    c2.backward(dC, g2d, overwrite=True, phase="params")                            # the frame is still there
    assert i2.any()


# ---------------------------------------------------------------- 6. planted gaussians

def test_planted_gaussians_contribute_nothing():
    n, W, H, deg = 1000, 96, 64, 2
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 730)
    sc["means"][100] = cam.eye
    sc["means"][200] = (np.nan, 0.0, 0.0)
    sc["scales"][300] = 200.0
    keep = np.ones(n, bool); keep[[100, 200, 300]] = False
    for det in (False, True):
        ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=det)
        g = _frame(ctx, synthetic.make_dC(W, H, 730), deg)["g"]
        got = ctx.backward_camera()
        dm = ctx.grads_read(g, deg)["means"]
        assert np.isfinite(got).all() and got[:16].any() and not dm[~keep].any()
        _identity(got, dm, sc["means"], T, keep)


# ---------------------------------------------------------------- 7. active degree, background

def test_active_degree_below_the_stored_one_equals_the_truncated_model():
    n, W, H = 1500, 96, 64
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, 3, 740)
    dC = synthetic.make_dC(W, H, 740)
    full = _ctx(sc, cam, T, P, W, H, 3, deterministic=True)
    full.set_active_sh_degree(1)
    g = _frame(full, dC, 3)["g"]
    a = full.backward_camera()
    _identity(a, full.grads_read(g, 3)["means"], sc["means"], T)
    cut = dict(sc, shs=np.ascontiguousarray(sc["shs"][:, :4]))
    trunc = _ctx(cut, cam, T, P, W, H, 1, deterministic=True)
    _frame(trunc, dC, 1)
    b = trunc.backward_camera()
    assert a[32:38].any() and same_bits(a, b)
    full.set_active_sh_degree(-1)
    _frame(full, dC, 3)
    assert not same_bits(full.backward_camera(), a)                                  # the higher bands do reach the camera


def test_background_colour():
    n, W, H, deg = 1500, 96, 64, 2
    sc, cam, T, P, _ = scene_and_cameras(n, W, H, deg, 750)
    dC = synthetic.make_dC(W, H, 750)
    outs = []
    for bg in (None, (0.3, 0.5, 0.7)):
        ctx = _ctx(sc, cam, T, P, W, H, deg, deterministic=True)
        if bg:
            ctx.set_background(bg)
        g = _frame(ctx, dC, deg)["g"]
        got = ctx.backward_camera()
        _identity(got, ctx.grads_read(g, deg)["means"], sc["means"], T)
        outs.append(got)
    assert outs[0][:16].any() and np.isfinite(outs[1]).all()


# ---------------------------------------------------------------- 8. it descends

DESCENT = dict(lr_eye=5e-3, iterations=150)


def test_pose_refinement_descends():
    """A frozen model, the eye displaced sideways by 1 % of its distance to lookAt (0.30 scene units, about two pixels of image motion);
    CameraAdam on the eye alone (lr_eye 5e-3, lookAt fixed so that the eye is identifiable), 150 iterations.  Reached on MI355X: loss
    0.001902 -> 0.000006, distance to the true eye 0.3017 -> 0.0009.
    Conditions: the final loss below the first, the eye's distance to the true eye under half the initial displacement."""
    from gaussiansplat_amd import optim, renderer as R, train as TR
    n, W, H, deg = 2000, 128, 96, 1
    sc = synthetic.make_scene(n, W, H, deg, seed=760)
    sc["scales"] = (sc["scales"] + np.float32(2.5)).astype(np.float32)              # splats a few pixels wide: a basin wider than the displacement
    true_cam = synthetic.scene_camera(W, 0)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, sc, deterministic=True, tile_parts=1)
    tps = R.preprocess(r, true_cam)
    R.compactIdxs(r)
    R.forward(r, tps)
    gt = r.imageData.clone()
    before = [t.clone() for t in (r.splatData.means, r.splatData.scales, r.splatData.quaternions, r.splatData.opacities, r.splatData.shs)]
    e, l = np.asarray(true_cam.eye, np.float64), np.asarray(true_cam.lookAt, np.float64)
    d0 = 0.01 * np.linalg.norm(l - e)
    start = dataclasses.replace(true_cam, eye=(e + d0 * np.array([0.8, -0.6, 0.0])).astype(np.float32))
    pose = optim.CameraAdam(start, DESCENT["lr_eye"], 0.0)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    losses = TR.train(r, gt, 0.0, lf, iterations=DESCENT["iterations"], pose=pose, freeze_model=True)
    dist = float(np.linalg.norm(np.asarray(pose.camera.eye, np.float64) - e))
    print(f"pose refinement: loss {losses[0]:.6f} -> {losses[-1]:.6f}, eye distance {d0:.4f} -> {dist:.4f}")
    assert pose.step_count == DESCENT["iterations"] and len(losses) == DESCENT["iterations"]
    assert losses[-1] < losses[0]
    assert dist < 0.5 * d0
    after = (r.splatData.means, r.splatData.scales, r.splatData.quaternions, r.splatData.opacities, r.splatData.shs)
    assert all(torch.equal(a, b) for a, b in zip(before, after))                    # frozen: the model did not move
