"""Loss + SGD step on the GPU against the loss.jl restatement and torch autograd."""
import os

import numpy as np
import pytest

import loss_ref as LR
from common import dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W,H", [(64, 48), (70, 37), (16, 16)])
def test_loss_and_gradient_match_oracle(W, H):
    import torch
    from gaussiansplat_amd import backend as B
    from oracle import loss_oracle_np as LO
    from test_loss import torch_loss
    rng = np.random.default_rng(W)
    img = rng.random((3, H, W), dtype=np.float32); gt = rng.random((3, H, W), dtype=np.float32)
    img[0, :3, :5] = gt[0, :3, :5]                                           # some exact ties: sign(0) = 0
    ctx = B.Context()
    loss, dC = ctx.loss_host(img, gt, 0.1)
    k = LO.kernel_window()
    assert abs(loss - LO.loss(img, gt, k)) <= 2e-6
    x = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    torch_loss(x, torch.tensor(gt, dtype=torch.float64), k).backward()
    want = x.grad.numpy()
    assert np.abs(dC - want).max() <= 1e-4 * np.abs(want).max() + 1e-9
    assert np.linalg.norm(dC - want) <= 1e-4 * np.linalg.norm(want)
    loss_same, dsame = ctx.loss_host(gt, gt, 0.1)
    assert abs(loss_same) < 1e-6
    ctx.close()


@pytest.mark.parametrize("W,H", [(1920, 1080), (1921, 1081)])
def test_loss_at_the_size_it_is_quoted_for(W, H):
    """The loss kernels own four outputs per thread, fold the 11 x 11 window to 6 x 6 weights and read LDS in 16-byte pieces
    (gs_loss.hip); they are timed at 1920x1080x3.  Parity at that size and at a ragged one (neither dimension a
    multiple of the kernels' tile): loss vs the loss.jl restatement, gradient vs fp64 torch autograd."""
    import torch
    from gaussiansplat_amd import backend as B
    from oracle import loss_oracle_np as LO
    from test_loss import torch_loss
    rng = np.random.default_rng(W * 7 + H)
    gt = rng.random((3, H, W), dtype=np.float32)
    img = np.clip(gt + 0.15 * rng.standard_normal((3, H, W)).astype(np.float32), 0.0, 1.0).astype(np.float32)    # a render near its target
    img[1, -7:, -9:] = gt[1, -7:, -9:]                                       # exact ties in the ragged corner: sign(0) = 0
    ctx = B.Context()
    loss, dC = ctx.loss_host(img, gt, 0.1)
    k = LO.kernel_window()
    assert abs(loss - LO.loss(img, gt, k)) <= 2e-6
    x = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    torch_loss(x, torch.tensor(gt, dtype=torch.float64), k, fft=True).backward()
    want = x.grad.numpy()
    assert np.abs(dC - want).max() <= 1e-4 * np.abs(want).max() + 1e-12
    assert np.linalg.norm(dC - want) <= 1e-4 * np.linalg.norm(want)
    # the borders see a truncated window: compare them on their own
    for sl in (np.s_[:, :6, :], np.s_[:, -6:, :], np.s_[:, :, :6], np.s_[:, :, -6:]):
        assert np.linalg.norm(dC[sl] - want[sl]) <= 1e-4 * np.linalg.norm(want[sl])
    ctx.close()


def test_sgd_step_and_training_reduces_loss():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    n, W, H, deg = 3000, 128, 96, 1
    gx, gy = W // 16, H // 16
    target = synthetic.make_scene(n, W, H, deg, seed=1)
    cam = synthetic.scene_camera(W)
    rt = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), target)
    R.forward(rt, (R.preprocess(rt, cam), R.compactIdxs(rt))[0])
    gt = rt.imageData.clone()
    start = {k: v.copy() for k, v in target.items()}
    start["shs"] = (start["shs"] + 0.2 * np.random.default_rng(2).standard_normal(start["shs"].shape)).astype(np.float32)
    start["opacities"] = (start["opacities"] - 0.5).astype(np.float32)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), start)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    before = r.splatData.shs.clone()
    # one step by hand: param_after == param_before - lr * grad
    tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
    l0, dC = lf.value_and_grad(r.imageData, gt)
    R.backward(r, dC)
    g = r.splatGrads.Δshs.clone()
    r._begin(); r.ctx.sgd_step(0.5, r._grads); torch.cuda.synchronize()
    assert torch.allclose(r.splatData.shs, before - 0.5 * g, rtol=1e-6, atol=1e-7)
    R.resetGrads(r)
    losses = TR.train(r, gt, 2.0, lf, iterations=25, camera=cam)
    assert losses[-1] < 0.95 * l0 and losses[-1] < losses[0], (l0, losses[0], losses[-1])   # plain SGD: slow but downhill
    assert all(np.isfinite(losses))


def test_fused_backward_sgd_equals_backward_then_sgd():
    """gs_backward_sgd updates the resident model exactly like gs_backward (overwrite) followed by gs_sgd_step: the same fma on
    the same float gradient, so the parameters agree bit for bit in deterministic mode."""
    import torch
    from gaussiansplat_amd import renderer as R, synthetic, train as TR
    n, W, H, deg = 4000, 160, 112, 3
    gx, gy = W // 16, H // 16
    scene = synthetic.make_scene(n, W, H, deg, seed=21)
    cam = synthetic.scene_camera(W)
    gt = torch.rand((3, H, W), device="cuda")
    out = []
    for fused in (False, True):
        r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), scene, deterministic=True)
        lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
        for _ in range(3):
            TR.trainStep(r, gt, 0.05, lf, cam, want_loss=False, fused_sgd=fused)
        torch.cuda.synchronize()
        sd = r.splatData
        out.append([x.clone() for x in (sd.means, sd.scales, sd.quaternions, sd.opacities, sd.shs)])
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][4], torch.as_tensor(scene["shs"]).reshape(out[0][4].shape).cuda())    # the model moved


@pytest.mark.parametrize("fused", [False, True])
def test_three_iteration_trajectory_against_an_oracle_side_loop(oracle, fused):
    """not only "the loss goes down".  Three iterations of train.jl:33-56 as intended -- render, loss (loss.jl:60-72),
    image gradient, backward, param .-= lr * grad -- run on the ORACLE side (oracle render with the same early-out, the loss.jl
    restatement differentiated by fp64 torch autograd, the fp64 adjoint, the update in float32) against train.trainStep x 3 in
    deterministic mode, plain and with the fused backward + SGD.  After step 3 every parameter array agrees to rel-L2 1e-4, and the
    DISPLACEMENT from the start (what the three gradients did; each gradient's own bar is 1e-3, and the second and third are taken on a
    frame re-rendered from the already displaced model) to 1e-2 -- measured 5e-3 on the quaternions, the most amplified chain, less
    elsewhere; the measured values go to gpurun_out/parity_sizes.json."""
    import torch
    from gaussiansplat_amd import camera as gcam, renderer as R, synthetic, train as TR
    from oracle import loss_oracle_np as LO
    from test_loss import torch_loss
    from common import rel_l2
    O = oracle
    n, W, H, deg, lr = 2500, 128, 96, 1, 8.0
    gx, gy = W // 16, H // 16
    scene = synthetic.make_scene(n, W, H, deg, seed=5)
    cam = synthetic.scene_camera(W)
    Tm, Pm = gcam.compute_transform(cam), gcam.compute_projection(cam, W, H)
    ocam = O.camera_from_arrays(Tm, Pm, np.float32(cam.fx), np.float32(cam.fy), np.float32(cam.near), np.float32(cam.far), cam.eye, cam.lookAt, W, H)
    gt = np.random.default_rng(6).random((3, H, W), dtype=np.float32)
    names = ("means", "scales", "quats", "opacities", "shs")
    p = {k: scene[k].copy() for k in names}
    kwin = LO.kernel_window()
    losses_o = []
    for _ in range(3):
        ref = O.render(p["means"], p["scales"], p["quats"], p["opacities"], p["shs"], deg, ocam, order=1, t_min=1e-5)
        x = torch.tensor(ref["image"], dtype=torch.float64, requires_grad=True)
        l = torch_loss(x, torch.tensor(gt, dtype=torch.float64), kwin)
        l.backward()
        losses_o.append(float(l))
        dC = x.grad.numpy().astype(np.float32)
        g = O.backward(p["means"], p["scales"], p["quats"], p["opacities"], p["shs"], deg, ocam, ref["ranges"], ref["ids"], dC, t_min=1e-5)
        for k in names:
            p[k] = (p[k] - np.float32(lr) * np.asarray(g[k]).reshape(p[k].shape).astype(np.float32)).astype(np.float32)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), (gx, gy), scene, deterministic=True)
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    gtd = torch.as_tensor(gt).cuda()
    losses_g = [TR.trainStep(r, gtd, lr, lf, cam, want_loss=True, fused_sgd=fused) for _ in range(3)]
    torch.cuda.synchronize()
    sd = r.splatData
    got = dict(means=sd.means, scales=sd.scales, quats=sd.quaternions, opacities=sd.opacities, shs=sd.shs)
    for a, b in zip(losses_g, losses_o):
        assert abs(a - b) <= 5e-6, (losses_g, losses_o)
    assert losses_o[2] < losses_o[0]
    rep = {}
    for k in names:
        a = got[k].cpu().numpy().astype(np.float64).reshape(-1)
        b, s0 = p[k].astype(np.float64).reshape(-1), scene[k].astype(np.float64).reshape(-1)
        moved = np.linalg.norm(b - s0)
        rep[k] = dict(param_rel_l2=rel_l2(a, b), displacement_rel_l2=float(np.linalg.norm(a - b) / max(moved, 1e-30)), displacement_over_param=float(moved / np.linalg.norm(s0)))
    from test_gpu_sizes import _report
    _report("trajectory_3_iterations" + ("_fused_sgd" if fused else ""), dict(lr=lr, losses_hip=losses_g, losses_oracle=losses_o, arrays=rep))
    for k in names:
        assert rep[k]["param_rel_l2"] <= 1e-4, (k, rep[k])
        assert rep[k]["displacement_over_param"] > 0.0, k
        assert rep[k]["displacement_rel_l2"] <= 1e-2, (k, rep[k])


# ---------------------------------------------------------------- the loss kernels on flat, smooth and tiny images (tests/loss_ref.py)
def _loss_device(ctx, img, gt, lam, want_dC=True, want_loss=True):
    """(loss, dC) through the device path: images and dC resident, dC filled with NaN first"""
    import torch
    Cn, H, W = img.shape
    x, y = dev(img), dev(gt)
    d = torch.full((Cn, H, W), float("nan"), device="cuda")
    loss = ctx.loss_device(x.data_ptr(), y.data_ptr(), d.data_ptr() if want_dC else 0, W, H, Cn, lam, want_loss)
    torch.cuda.synchronize()
    return loss, d.cpu().numpy()


@pytest.mark.parametrize("name", LR.FAMILIES)
def test_loss_family_within_the_float32_restatements_error(name):
    """Nine image families x lam in {0.1, 0.2, 1} x thirteen shapes (tests/loss_ref.py: below the window, one pixel wide, W % 4 == 3,
    either side of the 64 x 16 tile, exactly 8 tiles, other channel counts).  The kernel is compared with the float64 restatement
    and allowed 4 x the float32 restatement's own error on the same input: gradient max, gradient L2, loss, and the L2 of each
    border strip (the outer 6 rows / columns, the 6 columns either side of x = 64); loss_ref.RAISED names the parts of a family
    that are allowed up to 16 and why.  The measured ratios, kernel error over float32 error, go to the parity report of
    test_gpu_sizes._report (parity_sizes.json) under "loss_families"."""
    import json
    from gaussiansplat_amd import backend as B
    import test_gpu_sizes as TS
    ctx = B.Context()
    rep, bad = {}, []
    for lam in LR.LAMS:
        for shape in LR.SHAPES:
            img, gt, b = LR.case(name, shape, lam)
            loss, dC = ctx.loss_host(img, gt, lam)
            r = LR.ratios(dC, loss, b)
            rep["lam%g_%dx%dx%d" % ((lam,) + shape)] = r
            if not (np.isfinite(dC).all() and all(v <= LR.factor(name, shape, k) for k, v in r.items())):
                bad.append((lam, shape, r))
    ctx.close()
    rep["worst"] = {k: max(v[k] for v in rep.values()) for k in ("max", "l2", "loss", "strips")}
    print(name, json.dumps(rep["worst"]))
    prev = {}
    if os.path.exists(TS._REPORT):
        try:
            with open(TS._REPORT) as fh:
                prev = json.load(fh).get("loss_families", {})
        except Exception:
            prev = {}
    prev[name] = rep
    TS._report("loss_families", prev)
    assert not bad, bad


@pytest.mark.parametrize("name", ["uniform", "range"])
def test_loss_gradient_at_lambda_zero_is_the_l1_term_exactly(name):
    """lam = 0: the SSIM term is multiplied by -0.0, so dC = sign(img - gt) * (1 / (2 n)) in float32, element for element, and 0 at
    the planted ties"""
    from gaussiansplat_amd import backend as B
    ctx = B.Context()
    for shape in ((3, 17, 65), (5, 16, 67), (3, 2, 3)):
        img, gt, _ = LR.case(name, shape, 1.0)
        loss, dC = ctx.loss_host(img, gt, 0.0)
        want = np.sign(img - gt) * (np.float32(1.0) / (np.float32(2.0) * np.float32(img.size)))
        assert want.dtype == np.float32 and np.array_equal(dC, want), shape
        assert not dC[0, :3, :5].any()
        assert abs(loss - np.abs(img.astype(np.float64) - gt).sum() / (2.0 * img.size)) <= 1e-6 * loss
    ctx.close()


@pytest.mark.parametrize("name", ["uniform", "smooth_near"])
def test_loss_paths_agree_bit_for_bit(name):
    """dC has one writer per element and no atomics: bitwise equal across two runs, between the host and the device path, and with
    and without the loss read back.  With dC == NULL on the device path the loss is the one with a dC buffer to 1e-12 relative
    (the slotted double atomics may reorder)."""
    from gaussiansplat_amd import backend as B
    lam = 0.2
    img, gt, _ = LR.case(name, (3, 49, 193), lam)
    ctx = B.Context()
    loss_h, dC_h = ctx.loss_host(img, gt, lam)
    loss_h2, dC_h2 = ctx.loss_host(img, gt, lam)
    assert np.array_equal(dC_h, dC_h2) and abs(loss_h - loss_h2) <= 1e-12 * abs(loss_h)
    loss_d, dC_d = _loss_device(ctx, img, gt, lam)
    assert np.array_equal(dC_d, dC_h) and abs(loss_d - loss_h) <= 1e-12 * abs(loss_h)
    none, dC_q = _loss_device(ctx, img, gt, lam, want_loss=False)
    assert none is None and np.array_equal(dC_q, dC_h)
    loss_n, untouched = _loss_device(ctx, img, gt, lam, want_dC=False)
    assert abs(loss_n - loss_h) <= 1e-12 * abs(loss_h) and np.isnan(untouched).all()
    ctx.close()


@pytest.mark.parametrize("name", ["uniform", "smooth_near"])
@pytest.mark.parametrize("shape", [(3, 17, 65), (2, 33, 129)], ids=lambda s: "%dx%dx%d" % s)
def test_loss_symmetries(name, shape):
    """The loss is symmetric in its arguments, and the window under both reflections -- the tiling is not (tiles start at the top
    left, the ragged end is at the bottom right): dC of the flipped images is the flipped dC.  Every run is held to the bars of
    the unflipped case, against the float64 restatement of the unflipped case."""
    from gaussiansplat_amd import backend as B
    lam = 1.0
    img, gt, b = LR.case(name, shape, lam)
    ctx = B.Context()
    loss_swapped, _ = ctx.loss_host(gt, img, lam)
    assert abs(loss_swapped - b.loss) <= LR.factor(name, shape, "loss") * b.e_loss
    for flip in (np.s_[:, :, ::-1], np.s_[:, ::-1, :], np.s_[:, ::-1, ::-1]):
        loss, dC = ctx.loss_host(np.ascontiguousarray(img[flip]), np.ascontiguousarray(gt[flip]), lam)
        r = LR.ratios(dC[flip], loss, b)
        assert all(v <= LR.factor(name, shape, k) for k, v in r.items()), (flip, r)
    ctx.close()


def test_loss_context_reused_across_image_sizes():
    """One context runs a large image, a tiny one, another, and the large one again: its map planes still hold the larger
    image's maps.  Every dC equals a fresh context's bit for bit, the losses to 1e-12 relative."""
    from gaussiansplat_amd import backend as B
    lam = 0.2
    ctx = B.Context()
    for shape in ((3, 49, 193), (3, 2, 3), (1, 16, 64), (3, 49, 193)):
        img, gt, _ = LR.case("uniform", shape, lam)
        loss, dC = ctx.loss_host(img, gt, lam)
        fresh = B.Context()
        loss_f, dC_f = fresh.loss_host(img, gt, lam)
        fresh.close()
        assert np.array_equal(dC, dC_f), shape
        assert abs(loss - loss_f) <= 1e-12 * abs(loss_f), shape
    ctx.close()


def test_loss_refusals_leave_dC_untouched():
    """W, H or C <= 0, a bad mem, a NULL img or gt: GS_ERR_INVALID, and a sentinel-filled dC comes back as it went in"""
    import ctypes as C
    from gaussiansplat_amd import backend as B
    ctx = B.Context()
    img = np.full((3, 4, 5), 0.5, np.float32); gt = np.full((3, 4, 5), 0.25, np.float32)
    dC = np.full((3, 4, 5), -7.0, np.float32)
    out = C.c_double(-7.0)
    ip, gp = img.ctypes.data, gt.ctypes.data
    for ip_, gp_, W, H, Cn, mem in ((ip, gp, 0, 4, 3, B.GS_MEM_HOST), (ip, gp, 5, 0, 3, B.GS_MEM_HOST), (ip, gp, 5, 4, 0, B.GS_MEM_HOST),
                                    (ip, gp, -5, 4, 3, B.GS_MEM_HOST), (ip, gp, 5, -4, 3, B.GS_MEM_HOST), (ip, gp, 5, 4, -3, B.GS_MEM_HOST),
                                    (ip, gp, 5, 4, 3, 2), (ip, gp, 5, 4, 3, -1), (None, gp, 5, 4, 3, B.GS_MEM_HOST), (ip, None, 5, 4, 3, B.GS_MEM_HOST)):
        rc = ctx.L.gs_loss_l1_dssim(ctx.h, C.c_void_p(ip_), C.c_void_p(gp_), W, H, Cn, 0.2, C.c_void_p(dC.ctypes.data), C.byref(out), mem)
        assert rc == B.GS_ERR_INVALID, (W, H, Cn, mem, rc)
        assert np.all(dC == -7.0) and out.value == -7.0
    loss, got = ctx.loss_host(img, gt, 0.2)                                  # the context still works
    assert np.isfinite(loss) and np.isfinite(got).all()
    ctx.close()
