"""The per-view bilateral grid on the GPU (gs_bilagrid_apply / gs_bilagrid_backward / gs_bilagrid_tv / gs_bilagrid_adam,
appearance.BilateralGrid, train.trainStep(bilagrid=, view=)) against the NumPy restatement of tests/bilagrid_ref.py.

The bars.  The forward and the adjoint into the image are float32 statements, one rounding per operation: bit for bit (any NaN equals any
NaN: the cases carry a NaN sample).  The adjoint into the grid is, per float of a vertex, a sum of n double terms -- each float64(u) *
(float64(g) * float64(x)), the restatement's own bits -- rounded to float once:
    |d_grid - exact| <= c n_v 2^-53 A_v + 2^-24 |exact| + 2^-149        A_v = sum |t|,  exact = math.fsum(t)
n_v the pixels that touch the vertex and c the corners of one pixel that fall on one vertex (1; 2 per axis of a single vertex), so that
c n_v = n is the number of terms: (n - 1) u A bounds any order of summing n terms in double (u = 2^-53: the gather's per-lane chains and
its tree are one such order, and the lanes without a term add + 0, which is exact), the second term is the one rounding to float, the third
half the smallest float step.  Derived, not measured; every float of every vertex of every case is compared, and the largest share of the
bound that the device used is printed.  A vertex no pixel touches reads + 0.  The total variation is three such sums of squares:
|tv - exact| <= (N + 3) 2^-53 exact, N the squares of the longest sum (+ 3: the quotients and their two additions); its gradient is a
float32 statement: bit for bit.  The Adam step is gs_adam_step's statement (tests/adam_ref.py): bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import adam_ref as AR
import bilagrid_ref as BR
from common import render, same_bits, small_scene_renderer

pytestmark = pytest.mark.gpu

BIG = BR.SHAPES[5]                                                               # (300, 200, 16, 16, 8)
UNSTAGED = (41, 7, 32, 2, 24)                                                    # two y planes are 72 KiB: more than the pixel kernels stage in LDS
CASES = [(s, wt) for s in BR.SHAPES + [UNSTAGED] for wt in (False, True)]


@functools.lru_cache(maxsize=None)
def _ref(shape, weighted):
    """inputs and reference results of a case, computed once and shared (read-only)"""
    dims = shape[2:]
    x, d, G, w = BR.case(*shape, weighted)
    dG, A, n = BR.backward_grid(x, d, dims, w)
    r = dict(x=x, d=d, G=G, w=w, out=BR.forward(x, G, dims, w), dx=BR.backward_image(x, d, G, dims, w), dG=dG, A=A, n=n)
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


def _dev(a, off=0, dtype=np.float32):
    """an array on the device; off: floats past a 16-byte boundary its base pointer sits at (a view into a larger buffer)"""
    import torch
    a = np.array(a, dtype).reshape(-1)                                           # (a copy: the shared reference arrays are read-only)
    buf = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.as_tensor(a))
    assert t.data_ptr() % 16 == (4 * off) % 16
    return t


def _run(ctx, r, shape, off=0, in_place=False, want_dG=True):
    """apply and backward of a case through the C ABI: (out, d_img, d_grid or None) as arrays"""
    import torch
    W, H, dims = shape[0], shape[1], shape[2:]
    x, d, G = _dev(r["x"], off), _dev(r["d"], off), _dev(r["G"], off)
    w = _dev(r["w"], off) if r["w"] is not None else None
    out = _dev(np.full(3 * W * H, np.nan, np.float32), off)
    d_img = d if in_place else _dev(np.full(3 * W * H, np.nan, np.float32), off)
    dG = _dev(np.full(r["G"].size, np.nan, np.float32), off) if want_dG else None
    wp = w.data_ptr() if w is not None else 0
    ctx.bilagrid_apply(x.data_ptr(), G.data_ptr(), dims, wp, W, H, out.data_ptr())
    ctx.bilagrid_backward(x.data_ptr(), d.data_ptr(), G.data_ptr(), dims, wp, W, H, d_img.data_ptr(), dG.data_ptr() if want_dG else 0)
    ctx.synchronize()
    torch.cuda.synchronize()
    return (out.cpu().numpy().reshape(3, H, W), d_img.cpu().numpy().reshape(3, H, W), dG.cpu().numpy().reshape(-1, 12) if want_dG else None)


def _check_dG(dG, r, shape):
    exact, A, n = r["dG"], r["A"], r["n"]
    assert dG.dtype == np.float32 and dG.shape == exact.shape
    assert n.max() <= BR.terms_per_pixel(shape[2:]) * shape[0] * shape[1]
    nan = np.isnan(exact)
    assert np.array_equal(np.isnan(dG), nan)                                     # the vertices the NaN sample touches, and no other
    err = np.abs(dG.astype(np.float64) - exact)
    bound = BR.dG_bound(exact, A, n)
    print("d_grid error / bound, worst float: %.3g   (%d of %d vertices touched, %d floats NaN)"
          % (float((err / bound)[~nan].max()), int((n > 0).sum()), n.size, int(nan.sum())))
    assert np.all((err <= bound)[~nan]), (err[~nan].max(), bound[~nan].min())
    assert not dG[n == 0].view(np.uint32).any()                                  # untouched: + 0, the bits


@pytest.mark.parametrize("shape,weighted", CASES, ids=lambda v: str(v))
def test_bilagrid_against_the_restatement(ctx, shape, weighted):
    r = _ref(shape, weighted)
    out, d_img, dG = _run(ctx, r, shape)
    assert same_bits(out, r["out"], nan_equal=True)
    assert same_bits(d_img, r["dx"], nan_equal=True)
    _check_dG(dG, r, shape)
    _, in_place, dG2 = _run(ctx, r, shape, in_place=True)
    assert same_bits(in_place, d_img, nan_equal=True)                            # d_img == d_out: the same bits as written apart
    assert same_bits(dG2, dG, nan_equal=True)                                    # two calls, one of them in place: bit-equal
    _, no_dG, none = _run(ctx, r, shape, want_dG=False)
    assert none is None and same_bits(no_dG, d_img, nan_equal=True)              # d_grid == NULL: the same d_img bits
    _, no_dG_in_place, _ = _run(ctx, r, shape, in_place=True, want_dG=False)
    assert same_bits(no_dG_in_place, d_img, nan_equal=True)


@pytest.mark.parametrize("shape,weighted", CASES, ids=lambda v: str(v))
def test_bilagrid_with_every_base_four_bytes_past_a_16_byte_boundary(ctx, shape, weighted):
    """every case again with every buffer offset: the 4-byte path at sizes where the aligned call takes 16-byte accesses (80 x 56, 64 x 1,
    300 x 200) and at sizes where it never does"""
    r = _ref(shape, weighted)
    aligned = _run(ctx, r, shape)
    for in_place in (False, True):
        out, d_img, dG = _run(ctx, r, shape, off=1, in_place=in_place)
        assert same_bits(out, r["out"], nan_equal=True) and same_bits(d_img, r["dx"], nan_equal=True)
        assert same_bits(dG, aligned[2], nan_equal=True)                         # nothing of the gather depends on the alignment
    _, no_dG, _ = _run(ctx, r, shape, off=1, want_dG=False)
    assert same_bits(no_dG, r["dx"], nan_equal=True)


def test_bilagrid_gradient_does_not_depend_on_what_the_ctx_did_before():
    """a small case after a call at 300 x 200 on one ctx against a fresh ctx, and the large one again after the small: the same bits"""
    from gaussiansplat_amd import backend as B
    small_shape = BR.SHAPES[0]
    big, small = _ref(BIG, True), _ref(small_shape, True)
    used, fresh = B.Context(), B.Context()
    _run(used, big, BIG)
    a = _run(used, small, small_shape)
    b = _run(fresh, small, small_shape)
    again = _run(used, big, BIG)
    first = _run(fresh, big, BIG)
    used.close(); fresh.close()
    for p, q in zip(a + again, b + first):
        assert same_bits(p, q, nan_equal=True)
    _check_dG(a[2], small, small_shape)


# ---------------------------------------------------------------- total variation
@pytest.mark.parametrize("dims", [(4, 3, 2), (16, 16, 8), (3, 1, 4), (2, 5, 1), (1, 1, 1), (64, 2, 33)], ids=str)
def test_total_variation_value_and_gradient(ctx, dims):
    import torch
    rng = np.random.default_rng(sum(dims))
    G = BR.case(8, 8, *dims, False)[2]
    d0 = rng.standard_normal(G.size).astype(np.float32)
    Gd, dG, tv = _dev(G, 1), _dev(d0), torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    ctx.bilagrid_tv(Gd.data_ptr(), dims, 10.0, dG.data_ptr(), tv.data_ptr())
    ctx.synchronize(); torch.cuda.synchronize()
    exact, most = BR.tv_exact(G)
    got = float(tv.cpu()[0])
    print("tv %.17g, exact %.17g, error / bound %.3g" % (got, exact, abs(got - exact) / max((most + 3) * 2.0 ** -53 * exact, 1e-300)))
    assert abs(got - exact) <= (most + 3) * 2.0 ** -53 * exact
    assert same_bits(dG.cpu().numpy(), BR.tv_grad(G, 10.0, d0).reshape(-1))      # added to what d_grid held
    if max(dims) > 1:
        assert not same_bits(dG.cpu().numpy(), d0)
    ctx.bilagrid_tv(Gd.data_ptr(), dims, 10.0, dG.data_ptr(), 0)                 # again, without the value: it adds again
    ctx.bilagrid_tv(Gd.data_ptr(), dims, 0.0, 0, tv.data_ptr())                  # and the value alone: the same bits
    ctx.synchronize(); torch.cuda.synchronize()
    assert same_bits(dG.cpu().numpy(), BR.tv_grad(G, 10.0, BR.tv_grad(G, 10.0, d0)).reshape(-1))
    assert float(tv.cpu()[0]) == got


# ---------------------------------------------------------------- gs_bilagrid_adam
@pytest.mark.parametrize("dims", [(2, 2, 2), (16, 16, 8)], ids=str)
def test_bilagrid_adam_is_the_adam_step(ctx, dims):
    import torch
    rng = np.random.default_rng(3)
    n = 12 * dims[0] * dims[1] * dims[2]
    p, m, v = BR.identity(dims).reshape(-1), np.zeros(n, np.float32), np.zeros(n, np.float32)
    P, M, V = _dev(p, 1), _dev(m), _dev(v)
    lr, betas, eps = 2e-3, (0.9, 0.999), 1e-15
    for step, rate in ((1, lr), (2, lr), (3, 0.0)):
        g = rng.standard_normal(n).astype(np.float32)
        ctx.bilagrid_adam(P.data_ptr(), _keep(g).data_ptr(), M.data_ptr(), V.data_ptr(), n, rate, betas[0], betas[1], eps, step)
        ctx.synchronize(); torch.cuda.synchronize()
        h = AR.hyper([rate], betas[0], betas[1], eps, step)
        p2, m, v = AR.update(p, m, v, g, h, h["step_size"][0])
        if rate == 0.0:
            assert same_bits(p2, p)                                              # lr == 0 leaves the grid ...
        p = p2
        assert same_bits(P.cpu().numpy(), p) and same_bits(M.cpu().numpy(), m) and same_bits(V.cpu().numpy(), v)
    assert np.abs(p - BR.identity(dims).reshape(-1)).max() > 1e-3 and np.abs(m).max() > 0       # ... and still moves the moments


_KEEP = []


def _keep(a):
    """a device copy kept alive until the test module goes (the call that reads it is asynchronous)"""
    _KEEP.append(_dev(a))
    return _KEEP[-1]


# ---------------------------------------------------------------- the frame stays as it was
def test_bilagrid_calls_are_legal_anywhere_and_leave_the_frame_alone():
    """the four calls before any frame, between forward and backward of a real 300-gaussian frame and after the backward: imageData,
    splatGrads (the backward runs: the frame's stage is what it was) and the next frame, which inherits the view slot's history, come out as
    in a run without them, bit for bit (deterministic mode, one wave per tile)"""
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    runs = []
    for with_calls in (False, True):
        r, cam, W, H = small_scene_renderer(300, 5)
        shape = (W, H, 4, 3, 2)
        case = _ref(shape, True)
        dC = torch.as_tensor(synthetic.make_dC(W, H, 4)).cuda()

        def calls():
            if with_calls:
                out, d_img, dG = _run(r.ctx, case, shape)
                assert same_bits(out, case["out"], nan_equal=True) and same_bits(d_img, case["dx"], nan_equal=True)
                _check_dG(dG, case, shape)
                G, g, m, v = _dev(case["G"]), _dev(dG), _dev(np.zeros(dG.size)), _dev(np.zeros(dG.size))
                tv = torch.zeros(1, dtype=torch.float64, device="cuda")
                r.ctx.bilagrid_tv(G.data_ptr(), shape[2:], 10.0, g.data_ptr(), tv.data_ptr())
                r.ctx.bilagrid_adam(G.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), dG.size, 2e-3, 0.9, 0.999, 1e-15, 1)
                r.ctx.synchronize()
        r._begin()
        calls()                                                                  # before any frame: no model's frame, no camera's
        render(r, cam)
        image = r.imageData.clone()
        calls()                                                                  # between forward and backward
        R.backward(r, dC)
        grads = r.splatGrads.flat.clone()
        calls()                                                                  # after the backward
        torch.cuda.synchronize()
        assert torch.equal(image, r.imageData) and torch.equal(grads, r.splatGrads.flat)
        R.resetGrads(r)
        render(r, cam)                                                           # the next frame of the same view
        runs.append((image, grads, r.imageData.clone()))
    assert runs[0][1].abs().max() > 0
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- appearance.BilateralGrid
def test_bilateral_grid_steps_one_view_at_a_time():
    """apply / backward / step of views 2, 0, 2 on a 3-view table: the stepped grids and moments are the restatement's gradient (within its
    bound) plus the TV gradient through adam_ref at that VIEW's own step count; view 1 never changes; mask_target is w * gt exactly; a
    checkpoint carries everything"""
    import torch
    from gaussiansplat_amd.appearance import BilateralGrid
    r, cam, W, H = small_scene_renderer(300, 5)
    dims = (4, 3, 2)
    wgt = _ref((W, H, *dims), True)["w"]
    lr, betas, eps = 2e-3, (0.9, 0.999), 1e-15
    b = BilateralGrid(r, 3, grid=dims, weights=[None, None, wgt], lr=lr, tv_coef=10.0)
    rng = np.random.default_rng(17)
    table = np.tile(BR.identity(dims), (3, 1, 1, 1, 1))
    m, v, counts = np.zeros_like(table), np.zeros_like(table), [0, 0, 0]
    for view in (2, 0, 2):
        w = wgt if view == 2 else None
        x = rng.random((3, H, W)).astype(np.float32)
        d = rng.standard_normal((3, H, W)).astype(np.float32)
        out = b.apply(view, torch.as_tensor(x).cuda())
        assert same_bits(out.cpu().numpy(), BR.forward(x, table[view], dims, w))
        d_img = b.backward(view, torch.as_tensor(d).cuda())
        assert same_bits(d_img.cpu().numpy(), BR.backward_image(x, d, table[view], dims, w))
        g = b._grad.cpu().numpy().reshape(table[view].shape)
        b.step(view)
        counts[view] += 1
        h = AR.hyper([lr], betas[0], betas[1], eps, counts[view])
        table[view], m[view], v[view] = AR.update(table[view], m[view], v[view], g, h, h["step_size"][0])
        assert b.step_counts == counts
        assert same_bits(b.table.cpu().numpy(), table) and same_bits(b.exp_avg.cpu().numpy(), m) and same_bits(b.exp_avg_sq.cpu().numpy(), v)
    assert counts == [1, 0, 2] and np.array_equal(table[1], BR.identity(dims)) and not m[1].any()
    assert np.abs(table[2] - BR.identity(dims)).max() > 1e-3
    assert same_bits(b.grid(2), table[2])
    exact_tv, most = BR.tv_exact(table[2])
    assert abs(b.tv(2) - exact_tv) <= (most + 3) * 2.0 ** -53 * exact_tv and b.tv(1) == 0.0
    gt = torch.as_tensor(rng.random((3, H, W)).astype(np.float32)).cuda()
    assert b.mask_target(0, gt) is gt
    assert same_bits(b.mask_target(2, gt).cpu().numpy(), wgt[None] * (gt.cpu().numpy() + np.float32(0)))
    sd = b.state_dict()
    f = BilateralGrid(r, 3, grid=dims)
    f.load_state_dict(sd)
    assert torch.equal(f.table, b.table) and torch.equal(f.exp_avg, b.exp_avg) and torch.equal(f.exp_avg_sq, b.exp_avg_sq)
    assert f.step_counts == b.step_counts and f.lr == lr


def test_backward_adds_the_tv_gradient_to_the_data_gradient():
    """BilateralGrid.backward with tv_coef > 0 keeps gs_bilagrid_backward's d_grid with gs_bilagrid_tv's gradient added, bit for bit; with
    tv_coef == 0 the data gradient alone"""
    import torch
    from gaussiansplat_amd.appearance import BilateralGrid
    r, cam, W, H = small_scene_renderer(300, 5)
    dims = (4, 3, 2)
    case = _ref((W, H, *dims), False)
    grads = []
    for coef in (0.0, 10.0):
        b = BilateralGrid(r, 1, grid=dims, tv_coef=coef)
        b.table[0].copy_(torch.as_tensor(np.array(case["G"])))
        b.apply(0, torch.as_tensor(np.array(case["x"])).cuda())
        b.backward(0, torch.as_tensor(np.array(case["d"])).cuda())
        grads.append(b._grad.cpu().numpy())
    _check_dG(grads[0].reshape(-1, 12), case, (W, H, *dims))
    with np.errstate(invalid="ignore"):
        assert same_bits(grads[1], BR.tv_grad(case["G"], 10.0, grads[0]).reshape(-1), nan_equal=True)


# ---------------------------------------------------------------- refusals
def test_bilagrid_refusals_leave_the_outputs_untouched(ctx):
    """every refusal of include/gsplat.h: GS_ERR_INVALID, and sentinel-filled buffers come back as they went in"""
    import torch
    from gaussiansplat_amd import backend as B
    W, H, dims = 8, 4, (4, 3, 2)
    P, NF, S = W * H, 12 * 4 * 3 * 2, -7.0
    buf = torch.full((8 * P + 2 * NF,), S, dtype=torch.float32, device="cuda")   # overlapping views are cut from one buffer
    img, d_out = buf[0:3 * P], buf[3 * P:6 * P]
    out, wgt = torch.full((3 * P + NF,), S, device="cuda"), torch.full((P,), S, device="cuda")
    G, dG, m, v = (torch.full((NF,), S, device="cuda") for _ in range(4))
    tv = torch.full((1,), S, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off) if t is not None else None
    L, h = ctx.L, ctx.h
    huge = (32768, 21846)                                                        # 3 W H = 2^31 + 65536
    apply_cases = [
        (None, p(G), *dims, None, W, H, p(out)), (p(img), None, *dims, None, W, H, p(out)), (p(img), p(G), *dims, None, W, H, None),
        (p(img), p(G), *dims, None, 0, H, p(out)), (p(img), p(G), *dims, None, W, 0, p(out)), (p(img), p(G), *dims, None, -W, H, p(out)),
        (p(img), p(G), *dims, None, *huge, p(out)),
        (p(img), p(G), 0, 3, 2, None, W, H, p(out)), (p(img), p(G), 4, 65, 2, None, W, H, p(out)), (p(img), p(G), 4, 3, -1, None, W, H, p(out)),
        (p(img), p(G), *dims, None, W, H, p(img)), (p(img), p(G), *dims, None, W, H, p(img, 1)), (p(img), p(G), *dims, None, W, H, p(buf, 3 * P - 1)),
        (p(img), p(G), *dims, p(out, P), W, H, p(out)), (p(img), p(out, 3 * P), *dims, None, W, H, p(out, 1)),
    ]
    for a in apply_cases:
        assert L.gs_bilagrid_apply(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_bilagrid_apply(None, p(img), p(G), *dims, None, W, H, p(out)) == B.GS_ERR_INVALID
    d_img = out
    bwd_cases = [
        (None, p(d_out), p(G), *dims, None, W, H, p(d_img), p(dG)), (p(img), None, p(G), *dims, None, W, H, p(d_img), p(dG)),
        (p(img), p(d_out), None, *dims, None, W, H, p(d_img), p(dG)), (p(img), p(d_out), p(G), *dims, None, W, H, None, p(dG)),
        (p(img), p(d_out), p(G), *dims, None, 0, H, p(d_img), p(dG)), (p(img), p(d_out), p(G), *dims, None, W, -1, p(d_img), p(dG)),
        (p(img), p(d_out), p(G), *dims, None, *huge, p(d_img), p(dG)), (p(img), p(d_out), p(G), 4, 3, 0, None, W, H, p(d_img), p(dG)),
        (p(img), p(d_out), p(G), 65, 3, 2, None, W, H, p(d_img), p(dG)),
        (p(img), p(d_out), p(G), *dims, None, W, H, p(img), p(dG)), (p(img), p(d_out), p(G), *dims, None, W, H, p(img, 2 * P), p(dG)),   # d_img over img (and d_out)
        (p(img), p(d_out), p(G), *dims, p(d_img, 2 * P), W, H, p(d_img), p(dG)),                                                       # ... over the weight
        (p(img), p(d_out), p(d_img, 1), *dims, None, W, H, p(d_img), p(dG)),                                                           # ... over the grid
        (p(img), p(d_out), p(G), *dims, None, W, H, p(d_img), p(d_img, 3 * P - 1)),                                                    # ... over d_grid
        (p(img), p(d_out), p(G), *dims, None, W, H, p(d_out, 1), p(dG)), (p(img), p(d_out, 1), p(G), *dims, None, W, H, p(d_out), None),  # d_out, but not exactly
        (p(img), p(d_out), p(G), *dims, None, W, H, p(d_img), p(G, 5)), (p(img), p(d_out), p(G), *dims, None, W, H, p(d_img), p(buf, 3 * P - 1)),  # d_grid over an input
        (p(img), p(d_out), p(G), *dims, p(dG, NF - 1), W, H, p(d_img), p(dG)),
    ]
    for a in bwd_cases:
        assert L.gs_bilagrid_backward(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_bilagrid_backward(None, p(img), p(d_out), p(G), *dims, None, W, H, p(d_img), p(dG)) == B.GS_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    tv_cases = [
        (None, *dims, 10.0, p(dG), p(tv)), (p(G), 0, 3, 2, 10.0, p(dG), p(tv)), (p(G), 4, 3, 65, 10.0, p(dG), p(tv)),
        (p(G), *dims, -1.0, p(dG), p(tv)), (p(G), *dims, nan, p(dG), p(tv)), (p(G), *dims, inf, p(dG), p(tv)),
        (p(G), *dims, 10.0, p(G, 1), p(tv)), (p(G), *dims, 10.0, p(dG), p(G, 2)), (p(G), *dims, 10.0, p(dG), p(dG, NF - 2)),
    ]
    for a in tv_cases:
        assert L.gs_bilagrid_tv(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_bilagrid_tv(None, p(G), *dims, 10.0, p(dG), p(tv)) == B.GS_ERR_INVALID
    ok = (2e-3, 0.9, 0.999, 1e-15, 1)
    adam_cases = [
        (None, p(dG), p(m), p(v), NF, *ok), (p(G), None, p(m), p(v), NF, *ok), (p(G), p(dG), None, p(v), NF, *ok), (p(G), p(dG), p(m), None, NF, *ok),
        (p(G), p(dG), p(m), p(v), 0, *ok), (p(G), p(dG), p(m), p(v), -5, *ok), (p(G), p(dG), p(m), p(v), 12 * 64 ** 3 + 1, *ok),
        (p(G), p(dG), p(m), p(v), NF, 2e-3, 0.9, 0.999, 1e-15, 0), (p(G), p(dG), p(m), p(v), NF, 2e-3, 1.0, 0.999, 1e-15, 1),
        (p(G), p(dG), p(m), p(v), NF, 2e-3, 0.9, nan, 1e-15, 1), (p(G), p(dG), p(m), p(v), NF, 2e-3, 0.9, 0.999, 0.0, 1),
        (p(G), p(dG), p(m), p(v), NF, -2e-3, 0.9, 0.999, 1e-15, 1), (p(G), p(dG), p(m), p(v), NF, inf, 0.9, 0.999, 1e-15, 1),
        (p(G), p(dG), p(m), p(m), NF, *ok), (p(G), p(G), p(m), p(v), NF, *ok), (p(G), p(dG), p(G, NF - 1), p(v), NF, *ok),
    ]
    for a in adam_cases:
        assert L.gs_bilagrid_adam(h, *a) == B.GS_ERR_INVALID, a
    assert L.gs_bilagrid_adam(None, p(G), p(dG), p(m), p(v), NF, *ok) == B.GS_ERR_INVALID
    ctx.synchronize()
    torch.cuda.synchronize()
    for t in (buf, out, wgt, G, dG, m, v, tv):
        assert bool((t == S).all())
    shape = BR.SHAPES[0]                                                         # the context still works
    r = _ref(shape, True)
    o, dx, g = _run(ctx, r, shape)
    assert same_bits(o, r["out"], nan_equal=True) and same_bits(dx, r["dx"], nan_equal=True)


# ---------------------------------------------------------------- through train.trainStep
def _train_run(grid_of, iterations=2):
    import torch
    from gaussiansplat_amd import optim, train as TR
    r, cam, W, H = small_scene_renderer(300, 5)
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(9)).cuda()
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    opt = optim.Adam(r, lr=1e-2)
    b = grid_of(r)
    grads, losses = [], []
    for _ in range(iterations):
        kw = {} if b is None else dict(bilagrid=b, view=1)
        losses.append(TR.trainStep(r, gt, 0.0, lf, cam, optimizer=opt, **kw))
        grads.append(r._splatGrads.flat.cpu().numpy().copy())                   # what the backward left (resetGrads is lazy: not yet zeroed)
    d = r.splatData
    params = [t.cpu().numpy().copy() for t in (d.means, d.scales, d.quaternions, d.opacities, d.shs)]
    return grads, params, losses, b


def test_identity_grid_at_rate_zero_trains_exactly_as_without():
    """a BilateralGrid at identity with lr = 0, tv_coef = 0 and no weights: splatGrads after every backward and the stepped parameters are
    array_equal to a run without the argument (equal, not bit-equal: the stage turns -0 into +0)"""
    from gaussiansplat_amd.appearance import BilateralGrid
    g0, p0, l0, _ = _train_run(lambda r: None)
    g1, p1, l1, b = _train_run(lambda r: BilateralGrid(r, 3, lr=0.0, tv_coef=0.0))
    assert np.abs(g0[0]).max() > 0
    for a, c in zip(g0 + p0, g1 + p1):
        assert np.array_equal(a, c)
    assert l0 == l1
    assert b.step_counts == [0, 2, 0] and np.array_equal(b.table.cpu().numpy(), np.tile(BR.identity((16, 16, 8)), (3, 1, 1, 1, 1)))
    assert b.exp_avg.abs().max() > 0                                            # lr = 0 still moves the moments


def test_bilagrid_fit_recovers_a_known_vignette():
    """the target is the renderer's own image under a known smooth 4 x 4 x 2 grid (a vignette: the gain of every channel falls with the
    radius, the same on both luminance planes); the model is frozen; 200 iterations: the loss and the table's distance to the known grid
    both end below where they started (the values: DESIGN.md 5.8r)"""
    import torch
    from gaussiansplat_amd import train as TR
    from gaussiansplat_amd.appearance import BilateralGrid
    r, cam, W, H = small_scene_renderer(300, 5)
    render(r, cam)
    image = r.imageData.cpu().numpy()
    dims = (4, 4, 2)
    star = BR.identity(dims)
    yy, xx = np.meshgrid(np.linspace(-1, 1, 4), np.linspace(-1, 1, 4), indexing="ij")
    gain = (1.0 - 0.25 * (xx ** 2 + yy ** 2)).astype(np.float32)                # 1 at the centre, 0.5 in the corners
    for k in (0, 5, 10):
        star[:, :, :, k] = gain[None]
    gt = torch.as_tensor(BR.forward(image, star, dims)).cuda()
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    b = BilateralGrid(r, 1, grid=dims, lr=2e-3, tv_coef=0.0)
    start = float(np.abs(b.grid(0) - star).max())
    before = [t.clone() for t in (r.splatData.means, r.splatData.shs)]
    losses = TR.train(r, gt, 0.0, lf, iterations=200, camera=cam, freeze_model=True, bilagrid=b, view=0)
    err = float(np.abs(b.grid(0) - star).max())
    rms0 = float(np.sqrt(np.mean((BR.identity(dims) - star) ** 2))); rms = float(np.sqrt(np.mean((b.grid(0) - star) ** 2)))
    print("loss %.6g -> %.6g, |G - G*|_inf %.4g -> %.4g, rms %.4g -> %.4g" % (losses[0], losses[-1], start, err, rms0, rms))
    assert all(torch.equal(a, c) for a, c in zip(before, (r.splatData.means, r.splatData.shs)))
    assert b.step_counts == [200]
    assert losses[-1] < losses[0]
    assert rms < rms0


def test_bilagrid_beside_exposure_or_without_view_raises():
    import torch
    from gaussiansplat_amd import train as TR
    from gaussiansplat_amd.appearance import BilateralGrid, Exposure
    r, cam, W, H = small_scene_renderer(300, 5)
    gt = torch.zeros((3, H, W)).cuda()
    lf = TR.getLossFunction((W, H, 3), 11, 3, renderer=r)
    b, e = BilateralGrid(r, 2, grid=(4, 3, 2)), Exposure(r, 2)
    with pytest.raises(ValueError):
        TR.trainStep(r, gt, 0.0, lf, cam, bilagrid=b, exposure=e, view=0)
    with pytest.raises(ValueError):
        TR.trainStep(r, gt, 0.0, lf, cam, bilagrid=b)
    with pytest.raises(ValueError):
        TR.trainStep(r, gt, 0.0, lf, cam, view=0)
    with pytest.raises(ValueError):
        TR.trainStep(r, gt, 0.0, lf, cam, bilagrid=b, view=2)
    assert b.step_counts == [0, 0]
    assert TR.trainStep(r, gt, 0.0, lf, cam, bilagrid=b, view=1) is not None and b.step_counts == [0, 1]
