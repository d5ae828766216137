"""The per-view exposure stage on the GPU (gs_exposure_apply / gs_exposure_backward / gs_exposure_adam, appearance.Exposure,
train.trainStep(exposure=, view=)) against the NumPy restatement of tests/exposure_ref.py.

The bars.  The forward and the adjoint into the image are float32 statements, one rounding per operation: bit for bit.  The adjoint into
E is a sum of P = W H exact double terms, rounded to float once:
    |dE - exact| <= P 2^-53 A + 2^-24 |exact| + 2^-149        A = sum |t|
-- (P - 1) u A bounds any order of summing P exact terms in double (u = 2^-53), the second term is the one rounding to float, the third
half the smallest float step.  Derived, not measured; every entry of every case is compared.  The Adam step is gs_adam_step's statement
(tests/adam_ref.py): bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import adam_ref as AR
import exposure_ref as ER
from common import render, same_bits, small_scene_renderer

pytestmark = pytest.mark.gpu

CASES = [(W, H, wt) for (W, H) in ER.SHAPES for wt in (False, True)]


@functools.lru_cache(maxsize=None)
def _ref(W, H, weighted):
    """inputs and reference results of a case, computed once and shared (read-only)"""
    x, d, E, w = ER.case(W, H, weighted)
    dE, A = ER.backward_exposure(x, d, w)
    r = dict(x=x, d=d, E=E, w=w, out=ER.forward(x, E, w), dx=ER.backward_image(d, E, w), dE=dE, A=A)
    for a in r.values():
        if a is not None:
            a.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def ctx():
    from gaussiansplat_amd import backend as B
    c = B.Context()
    yield c
    c.close()


def _dev(a, off=0):
    """a float32 array on the device; off: floats past a 16-byte boundary its base pointer sits at (a view into a larger buffer)"""
    import torch
    a = np.array(a, np.float32).reshape(-1)                                  # (a copy: the shared reference arrays are read-only)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.as_tensor(a))
    assert t.data_ptr() % 16 == 4 * off
    return t


def _run(ctx, r, W, H, off=0, in_place=False, want_dE=True):
    """apply and backward of a case through the C ABI: (out, d_img, dE or None) as arrays"""
    import torch
    x, d, E = _dev(r["x"], off), _dev(r["d"], off), _dev(r["E"], off)
    w = _dev(r["w"], off) if r["w"] is not None else None
    out = _dev(np.full(3 * W * H, np.nan, np.float32), off)
    d_img = d if in_place else _dev(np.full(3 * W * H, np.nan, np.float32), off)
    dE = _dev(np.full(12, np.nan, np.float32), off) if want_dE else None
    wp = w.data_ptr() if w is not None else 0
    ctx.exposure_apply(x.data_ptr(), E.data_ptr(), wp, W, H, out.data_ptr())
    ctx.exposure_backward(x.data_ptr(), d.data_ptr(), E.data_ptr(), wp, W, H, d_img.data_ptr(), dE.data_ptr() if want_dE else 0)
    ctx.synchronize()
    torch.cuda.synchronize()
    return (out.cpu().numpy().reshape(3, H, W), d_img.cpu().numpy().reshape(3, H, W),
            dE.cpu().numpy().reshape(3, 4) if want_dE else None)


def _check_dE(dE, r, W, H):
    err = np.abs(dE.astype(np.float64) - r["dE"])
    bound = ER.dE_bound(r["dE"], r["A"], W * H)
    print("dE error / bound, worst entry: %.3g" % float((err / bound).max()))
    assert dE.dtype == np.float32 and np.isfinite(dE).all()
    assert np.all(err <= bound), (err, bound)


@pytest.mark.parametrize("W,H,weighted", CASES, ids=lambda v: str(v))
def test_exposure_against_the_restatement(ctx, W, H, weighted):
    r = _ref(W, H, weighted)
    out, d_img, dE = _run(ctx, r, W, H)
    assert same_bits(out, r["out"])
    assert same_bits(d_img, r["dx"])
    _check_dE(dE, r, W, H)
    _, in_place, dE2 = _run(ctx, r, W, H, in_place=True)
    assert same_bits(in_place, d_img)                                        # d_img == d_out: the same bits as written apart
    assert same_bits(dE2, dE)                                                # two calls: bit-equal
    _, no_dE, none = _run(ctx, r, W, H, want_dE=False)
    assert none is None and same_bits(no_dE, d_img)                          # d_exposure == NULL: the same d_img bits
    _, no_dE_in_place, _ = _run(ctx, r, W, H, in_place=True, want_dE=False)
    assert same_bits(no_dE_in_place, d_img)


@pytest.mark.parametrize("W,H,weighted", [(129, 33, True), (129, 33, False), (320, 200, True), (320, 200, False)], ids=lambda v: str(v))
def test_exposure_with_every_base_four_bytes_past_a_16_byte_boundary(ctx, W, H, weighted):
    """the scalar path at a size where the aligned call takes 16-byte accesses (320 x 200), and at one where it never does (129 x 33)"""
    r = _ref(W, H, weighted)
    aligned = _run(ctx, r, W, H)
    for in_place in (False, True):
        out, d_img, dE = _run(ctx, r, W, H, off=1, in_place=in_place)
        assert same_bits(out, r["out"]) and same_bits(d_img, r["dx"])
        _check_dE(dE, r, W, H)
        assert same_bits(dE, aligned[2])                                     # the pixel -> lane mapping does not depend on the alignment
    _, no_dE, _ = _run(ctx, r, W, H, off=1, want_dE=False)
    assert same_bits(no_dE, r["dx"])


def test_exposure_gradient_does_not_depend_on_what_the_ctx_did_before():
    """(129, 33) after a call at (320, 200) on one ctx -- the larger call's partial rows are still behind the smaller one's -- against a
    fresh ctx: the same bits"""
    from gaussiansplat_amd import backend as B
    big, small = _ref(320, 200, True), _ref(129, 33, True)
    used, fresh = B.Context(), B.Context()
    _run(used, big, 320, 200)
    a = _run(used, small, 129, 33)
    b = _run(fresh, small, 129, 33)
    again = _run(used, big, 320, 200)
    first = _run(fresh, big, 320, 200)
    used.close(); fresh.close()
    for p, q in zip(a + again, b + first):
        assert same_bits(p, q)
    _check_dE(a[2], small, 129, 33)


# ---------------------------------------------------------------- the frame stays as it was
def test_exposure_calls_are_legal_anywhere_and_leave_the_frame_alone():
    """apply and backward before any frame, between forward and backward of a real frame and after the backward: imageData and
    splatGrads come out as in a run without them, bit for bit (deterministic mode, one wave per tile)"""
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    runs = []
    for with_calls in (False, True):
        r, cam, W, H = small_scene_renderer(300, 5)
        case = _ref(W, H, True)
        dC = torch.as_tensor(synthetic.make_dC(W, H, 4)).cuda()

        def calls():
            if with_calls:
                out, d_img, dE = _run(r.ctx, case, W, H)
                assert same_bits(out, case["out"]) and same_bits(d_img, case["dx"])
                _check_dE(dE, case, W, H)
        r._begin()
        calls()                                                              # before any frame: no model's frame, no camera's
        render(r, cam)
        image = r.imageData.clone()
        calls()                                                              # between forward and backward
        R.backward(r, dC)
        grads = r.splatGrads.flat.clone()
        calls()                                                              # after the backward
        torch.cuda.synchronize()
        assert torch.equal(image, r.imageData) and torch.equal(grads, r.splatGrads.flat)
        runs.append((image, grads))
    assert runs[0][1].abs().max() > 0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------- gs_exposure_adam, through appearance.Exposure
def test_exposure_adam_steps_one_view_at_a_time():
    """five steps on a 4-view table, views 2, 0, 2, 2, 3, fresh random gradients: the stepped rows and their moments are adam_ref.update
    with adam_ref.hyper at that VIEW's own step count, bit for bit; view 1's row, moments and count never change"""
    import torch
    from gaussiansplat_amd.appearance import Exposure
    r, cam, W, H = small_scene_renderer(300, 5)
    lr, betas, eps = 0.01, (0.9, 0.999), 1e-15
    e = Exposure(r, 4, lr=lr, betas=betas, eps=eps)
    rng = np.random.default_rng(17)
    table = np.tile(ER.identity(), (4, 1, 1))
    m, v, counts = np.zeros((4, 3, 4), np.float32), np.zeros((4, 3, 4), np.float32), [0, 0, 0, 0]
    for view in (2, 0, 2, 2, 3):
        x = rng.standard_normal((3, H, W)).astype(np.float32)
        d = rng.standard_normal((3, H, W)).astype(np.float32)
        out = e.apply(view, torch.as_tensor(x).cuda())
        assert same_bits(out.cpu().numpy(), ER.forward(x, table[view]))
        e.backward(view, torch.as_tensor(d).cuda())
        g = e._grad.cpu().numpy().reshape(3, 4)
        exact, A = ER.backward_exposure(x, d, None)
        assert np.all(np.abs(g.astype(np.float64) - exact) <= ER.dE_bound(exact, A, W * H))
        e.step(view)
        counts[view] += 1
        h = AR.hyper([lr], betas[0], betas[1], eps, counts[view])
        table[view], m[view], v[view] = AR.update(table[view], m[view], v[view], g, h, h["step_size"][0])
        assert e.step_counts == counts
        assert same_bits(e.table.cpu().numpy(), table) and same_bits(e.exp_avg.cpu().numpy(), m) and same_bits(e.exp_avg_sq.cpu().numpy(), v)
    assert counts == [1, 0, 3, 1] and np.array_equal(table[1], ER.identity()) and not m[1].any() and not v[1].any()
    assert np.abs(table[2] - ER.identity()).max() > 0.02                    # three steps of about the rate each
    assert same_bits(e.exposure(2), table[2])
    # lr = 0 keeps the row and moves the moments
    e.set_lr(0.0)
    x = rng.standard_normal((3, H, W)).astype(np.float32); d = rng.standard_normal((3, H, W)).astype(np.float32)
    e.apply(2, torch.as_tensor(x).cuda()); e.backward(2, torch.as_tensor(d).cuda()); g = e._grad.cpu().numpy().reshape(3, 4); e.step(2)
    h = AR.hyper([0.0], betas[0], betas[1], eps, 4)
    p2, m2, v2 = AR.update(table[2], m[2], v[2], g, h, h["step_size"][0])
    assert same_bits(p2, table[2]) and not same_bits(m2, m[2]) and not same_bits(v2, v[2])
    assert same_bits(e.exposure(2), table[2]) and same_bits(e.exp_avg[2].cpu().numpy(), m2) and same_bits(e.exp_avg_sq[2].cpu().numpy(), v2)
    assert e.step_counts == [1, 0, 4, 1]
    # a checkpoint carries the table, the moments, the counts and the rate
    sd = e.state_dict()
    f = Exposure(r, 4)
    f.load_state_dict(sd)
    assert torch.equal(f.table, e.table) and torch.equal(f.exp_avg, e.exp_avg) and torch.equal(f.exp_avg_sq, e.exp_avg_sq)
    assert f.step_counts == e.step_counts and f.lr == 0.0


def test_mask_target_is_the_weight_times_the_target_exactly():
    import torch
    from gaussiansplat_amd.appearance import Exposure
    r, cam, W, H = small_scene_renderer(300, 5)
    case = _ref(W, H, True)
    e = Exposure(r, 2, weights=[None, case["w"]])
    gt = torch.as_tensor(np.array(case["x"])).cuda()
    assert e.mask_target(0, gt) is gt
    masked = e.mask_target(1, gt).cpu().numpy()
    assert same_bits(masked, case["w"][None] * (case["x"] + np.float32(0)))
    out = e.apply(1, gt).cpu().numpy()                                       # the table's identity row with the view's weight: the same
    assert same_bits(out, masked)


# ---------------------------------------------------------------- refusals
def test_exposure_refusals_leave_the_outputs_untouched(ctx):
    """every refusal of include/gsplat.h: GS_ERR_INVALID, and sentinel-filled outputs come back as they went in"""
    import torch
    from gaussiansplat_amd import backend as B
    W, H = 8, 4
    P = W * H
    S = -7.0
    buf = torch.full((8 * P,), S, dtype=torch.float32, device="cuda")        # overlapping views are cut from one buffer
    img, d_out, out, wgt = buf[0:3 * P], buf[3 * P:6 * P], torch.full((3 * P,), S, device="cuda"), torch.full((P,), S, device="cuda")
    E = torch.full((12,), S, device="cuda"); dE = torch.full((12,), S, device="cuda")
    m = torch.full((12,), S, device="cuda"); v = torch.full((12,), S, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off) if t is not None else None
    L, h = ctx.L, ctx.h
    huge = (32768, 21846)                                                    # 3 W H = 2^31 + 65536
    apply_cases = [
        (None, p(E), None, W, H, p(out)), (p(img), None, None, W, H, p(out)), (p(img), p(E), None, W, H, None),
        (p(img), p(E), None, 0, H, p(out)), (p(img), p(E), None, W, 0, p(out)), (p(img), p(E), None, -W, H, p(out)), (p(img), p(E), None, W, -H, p(out)),
        (p(img), p(E), None, *huge, p(out)),
        (p(img), p(E), None, W, H, p(img)), (p(img), p(E), None, W, H, p(img, 1)), (p(img), p(E), None, W, H, p(buf, 3 * P - 1)),
        (p(img), p(E), p(out, P), W, H, p(out)), (p(img), p(E), p(out, 3 * P - 1), W, H, p(out)),
        (p(img), p(out, 5), None, W, H, p(out)), (p(img), p(out, 3 * P - 1), None, W, H, p(out)),
    ]
    for a in apply_cases:
        assert L.gs_exposure_apply(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_exposure_apply(None, p(img), p(E), None, W, H, p(out)) == B.GS_ERR_INVALID
    d_img = out
    bwd_cases = [
        (None, p(d_out), p(E), None, W, H, p(d_img), p(dE)), (p(img), None, p(E), None, W, H, p(d_img), p(dE)),
        (p(img), p(d_out), None, None, W, H, p(d_img), p(dE)), (p(img), p(d_out), p(E), None, W, H, None, p(dE)),
        (p(img), p(d_out), p(E), None, 0, H, p(d_img), p(dE)), (p(img), p(d_out), p(E), None, W, -1, p(d_img), p(dE)),
        (p(img), p(d_out), p(E), None, *huge, p(d_img), p(dE)),
        (p(img), p(d_out), p(E), None, W, H, p(img), p(dE)), (p(img), p(d_out), p(E), None, W, H, p(img, 2 * P), p(dE)),      # d_img over img (and d_out)
        (p(img), p(d_out), p(E), p(d_img, 2 * P), W, H, p(d_img), p(dE)),                                                    # ... over the weight
        (p(img), p(d_out), p(d_img, 1), None, W, H, p(d_img), p(dE)),                                                        # ... over exposure
        (p(img), p(d_out), p(E), None, W, H, p(d_img), p(d_img, 3 * P - 12)),                                                # ... over d_exposure
        (p(img), p(d_out), p(E), None, W, H, p(d_out, 1), p(dE)), (p(img), p(d_out, 1), p(E), None, W, H, p(d_out), None),    # d_out, but not exactly
        (p(img), p(buf, 7 * P), p(E), None, W, H, p(buf, 5 * P), p(dE)),
    ]
    for a in bwd_cases:
        assert L.gs_exposure_backward(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_exposure_backward(None, p(img), p(d_out), p(E), None, W, H, p(d_img), p(dE)) == B.GS_ERR_INVALID
    ok = (0.01, 0.9, 0.999, 1e-15, 1)
    nan, inf = float("nan"), float("inf")
    adam_cases = [
        (None, p(dE), p(m), p(v), *ok), (p(E), None, p(m), p(v), *ok), (p(E), p(dE), None, p(v), *ok), (p(E), p(dE), p(m), None, *ok),
        (p(E), p(dE), p(m), p(v), 0.01, 0.9, 0.999, 1e-15, 0), (p(E), p(dE), p(m), p(v), 0.01, 0.9, 0.999, 1e-15, -3),
        (p(E), p(dE), p(m), p(v), 0.01, 1.0, 0.999, 1e-15, 1), (p(E), p(dE), p(m), p(v), 0.01, -0.1, 0.999, 1e-15, 1),
        (p(E), p(dE), p(m), p(v), 0.01, 0.9, 1.0, 1e-15, 1), (p(E), p(dE), p(m), p(v), 0.01, 0.9, nan, 1e-15, 1),
        (p(E), p(dE), p(m), p(v), 0.01, 0.9, 0.999, 0.0, 1), (p(E), p(dE), p(m), p(v), 0.01, 0.9, 0.999, -1e-8, 1),
        (p(E), p(dE), p(m), p(v), 0.01, 0.9, 0.999, inf, 1), (p(E), p(dE), p(m), p(v), 0.01, 0.9, 0.999, nan, 1),
        (p(E), p(dE), p(m), p(v), -0.01, 0.9, 0.999, 1e-15, 1), (p(E), p(dE), p(m), p(v), inf, 0.9, 0.999, 1e-15, 1),
        (p(E), p(dE), p(m), p(v), nan, 0.9, 0.999, 1e-15, 1),
        (p(E), p(dE), p(m), p(m), *ok), (p(E), p(E), p(m), p(v), *ok), (p(E), p(dE), p(E, 11), p(v), *ok), (p(buf, 4), p(dE), p(m), p(buf, 15), *ok),
    ]
    for a in adam_cases:
        assert L.gs_exposure_adam(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_exposure_adam(None, p(E), p(dE), p(m), p(v), *ok) == B.GS_ERR_INVALID
    ctx.synchronize()
    torch.cuda.synchronize()
    for t in (buf, out, wgt, E, dE, m, v):
        assert bool((t == S).all())
    r = _ref(5, 7, True)                                                     # the context still works
    o, dx, g = _run(ctx, r, 5, 7)
    assert same_bits(o, r["out"]) and same_bits(dx, r["dx"])


# ---------------------------------------------------------------- through train.trainStep
def _train_run(exposure_of, iterations=2):
    import torch
    from gaussiansplat_amd import optim, train as TR
    r, cam, W, H = small_scene_renderer(300, 5)
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(9)).cuda()
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    opt = optim.Adam(r, lr=1e-2)
    e = exposure_of(r)
    grads, losses = [], []
    for _ in range(iterations):
        kw = {} if e is None else dict(exposure=e, view=1)
        losses.append(TR.trainStep(r, gt, 0.0, lf, cam, optimizer=opt, **kw))
        grads.append(r._splatGrads.flat.cpu().numpy().copy())               # what the backward left (resetGrads is lazy: not yet zeroed)
    d = r.splatData
    params = [t.cpu().numpy().copy() for t in (d.means, d.scales, d.quaternions, d.opacities, d.shs)]
    return grads, params, losses, e


def test_identity_exposure_at_rate_zero_trains_exactly_as_without():
    """an Exposure at identity with lr = 0 and no weights: splatGrads after every backward and the stepped parameters are array_equal to a
    run without the argument (equal, not bit-equal: the stage turns -0 into +0)"""
    from gaussiansplat_amd.appearance import Exposure
    g0, p0, l0, _ = _train_run(lambda r: None)
    g1, p1, l1, e = _train_run(lambda r: Exposure(r, 3, lr=0.0))
    assert np.abs(g0[0]).max() > 0
    for a, b in zip(g0 + p0, g1 + p1):
        assert np.array_equal(a, b)
    assert l0 == l1
    assert e.step_counts == [0, 2, 0] and np.array_equal(e.table.cpu().numpy(), np.tile(ER.identity(), (3, 1, 1)))
    assert e.exp_avg.abs().max() > 0                                        # lr = 0 still moves the moments


def test_masked_step_compares_the_masked_images_and_the_fused_optimiser_follows():
    """a view with a weight: the loss of the step is the loss of (w img, w gt) formed by hand; and a fused optim.Adam behind the stage
    leaves the parameters of the unfused one, bit for bit (the contract of gs_backward_adam: it only ever sees a dC)"""
    import torch
    from gaussiansplat_amd import optim, train as TR
    from gaussiansplat_amd.appearance import Exposure
    w = _ref(64, 48, True)["w"]
    params = []
    for fused in (False, True):
        r, cam, W, H = small_scene_renderer(300, 5)
        gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(9)).cuda()
        lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
        e = Exposure(r, 2, weights=[None, w])
        if not fused:
            render(r, cam)
            wt = torch.as_tensor(np.array(w)).cuda()
            by_hand = lf(wt[None] * r.imageData, wt[None] * gt)
        opt = optim.Adam(r, lr=1e-2, fused=fused)
        losses = [TR.trainStep(r, gt, 0.0, lf, cam, optimizer=opt, exposure=e, view=1) for _ in range(2)]
        if not fused:
            assert losses[0] == by_hand
        d = r.splatData
        params.append([t.cpu().numpy().copy() for t in (d.means, d.scales, d.quaternions, d.opacities, d.shs)] + [e.table.cpu().numpy(), np.array(losses)])
        assert e.step_counts == [0, 2] and np.abs(e.exposure(1) - ER.identity()).max() > 0.005
    for a, b in zip(*params):
        assert same_bits(a, b)


def test_exposure_fit_recovers_a_known_affine():
    """the target is the renderer's own image under a known E* with |E* - [I | 0]|_inf = 0.2; the model is frozen; 200 iterations at
    lr = 0.01 -- 200 steps of at most about the rate each, ten times the distance to travel: the loss ends below where it started and
    |E - E*|_inf ends below 0.2"""
    import torch
    from gaussiansplat_amd import train as TR
    from gaussiansplat_amd.appearance import Exposure
    r, cam, W, H = small_scene_renderer(300, 5)
    render(r, cam)
    image = r.imageData.cpu().numpy()
    star = (ER.identity() + np.array([[0.2, -0.05, 0.1, 0.05], [0.1, -0.2, 0.05, -0.1], [-0.1, 0.15, 0.2, 0.1]], np.float32)).astype(np.float32)
    assert abs(float(np.abs(star - ER.identity()).max()) - 0.2) < 1e-7
    gt = torch.as_tensor(ER.forward(image, star)).cuda()
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    e = Exposure(r, 1, lr=0.01)
    before = [t.clone() for t in (r.splatData.means, r.splatData.shs)]
    losses = TR.train(r, gt, 0.0, lf, iterations=200, camera=cam, freeze_model=True, exposure=e, view=0)
    err = float(np.abs(e.exposure(0) - star).max())
    print("loss %.6g -> %.6g, |E - E*|_inf 0.2 -> %.4g" % (losses[0], losses[-1], err))
    assert all(torch.equal(a, b) for a, b in zip(before, (r.splatData.means, r.splatData.shs)))
    assert e.step_counts == [200]
    assert losses[-1] < losses[0]
    assert err < 0.2
