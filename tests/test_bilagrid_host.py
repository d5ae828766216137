"""The per-view bilateral grid without a GPU: the statements of csrc/gs_bilagrid.h in a host build (tests/bilagrid_host.cpp) against the
NumPy restatement (tests/bilagrid_ref.py), bit for bit; the restatement against torch's grid_sample formulation in float64 with autograd;
the argument checks of appearance.BilateralGrid and of train.trainStep's bilagrid / view pair that need no device.

The bars against torch.  torch.nn.functional.grid_sample(bilinear, border, align_corners=True) over (c / (W - 1),
r / (H - 1), clamp(l, 0, 1)) followed by the affine, in float64, is the yardstick; the restatement is float32.  Its worst error on the five
shapes below, seed 0, was measured once -- forward 7.1e-7 absolute (values about 1.5); d_img 1.12e-5 absolute at |d| ~ 1, the guidance term
included; d_grid 9.6e-7 of the largest entry, all three at (80, 56, 16, 16, 8) -- and four times that is allowed for every seed: FWD_BAR,
DIMG_BAR, DGRID_BAR.  Every pixel and every float of every vertex is compared."""
import subprocess

import numpy as np
import pytest

import bilagrid_ref as BR
from common import host_program, run_host, same_bits

HOST_SHAPES = BR.SHAPES[:5]                                                      # every shape but the 300 x 200 one
UNSTAGED = (41, 7, 32, 2, 24)                                                    # the grid the GPU's pixel kernels read without staging it
FWD_BAR, DIMG_BAR, DGRID_BAR = 4 * 7.1e-7, 4 * 1.12e-5, 4 * 9.6e-7


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program("bilagrid", tmp_path_factory.mktemp("bilagrid_host"))


def _run_host(host_exe, x, d, G, dims, w=None, coef=0.0, d_grid0=None):
    _, H, W = x.shape
    n, nf = 3 * H * W, G.size
    d0 = np.zeros(nf, np.float32) if d_grid0 is None else d_grid0
    head = np.array([W, H, *dims, int(w is not None)], np.int32).tobytes() + np.float32(coef).tobytes()
    arrays = [np.asarray(a, np.float32) for a in (G, d0, x, d) + ((w,) if w is not None else ())]
    out, dx, vertex, terms, tv, dg = run_host(host_exe, [], head, arrays, [(np.float32, n), (np.float32, n), (np.int32, 8 * H * W),
                                                                          (np.float64, 96 * H * W), (np.float64, 1), (np.float32, nf)])
    return out.reshape(3, H, W), dx.reshape(3, H, W), vertex.reshape(8, H * W), terms.reshape(8, H * W, 12), tv[0], dg.reshape(G.shape)


def _weights(W, H, dims):
    """None, the random weight of the cases (zeros and ones among it), and one of zeros and ones only"""
    rng = np.random.default_rng(W + 31 * H)
    return [None, BR.case(W, H, *dims, True)[3], (rng.random((H, W)) < 0.5).astype(np.float32)]


@pytest.mark.parametrize("shape", HOST_SHAPES + [UNSTAGED], ids=str)
def test_header_statements_equal_the_restatement_bit_for_bit(host_exe, shape):
    W, H, dims = shape[0], shape[1], shape[2:]
    x, d, G, _ = BR.case(*shape, False)                                          # with the -0 pixel and the NaN sample
    d0 = np.random.default_rng(5).standard_normal(G.size).astype(np.float32)
    for w in _weights(W, H, dims):
        out, dx, vertex, terms, tv, dg = _run_host(host_exe, x, d, G, dims, w, coef=10.0, d_grid0=d0)
        assert same_bits(out, BR.forward(x, G, dims, w), nan_equal=True)
        assert same_bits(dx, BR.backward_image(x, d, G, dims, w), nan_equal=True)
        rv, rt = BR.terms(x, d, dims, w)
        assert same_bits(vertex, rv)
        # the program reads a term off an accumulator that started at + 0: -0 comes as +0
        assert same_bits(terms, rt + 0.0, nan_equal=True)
        assert same_bits(np.float64(tv), BR.tv(G))
        assert same_bits(dg, BR.tv_grad(G, 10.0, d0))
    assert np.isnan(out[:, H // 2, W // 2]).all() and np.isfinite(np.delete(out.reshape(3, -1), (H // 2) * W + W // 2, axis=1)).all()


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_identity_grid_returns_the_image_and_masks_exactly(host_exe, shape):
    W, H, dims = shape[0], shape[1], shape[2:]
    x, d, _, _ = BR.case(*shape, False, special=False)
    x.reshape(-1)[:3] = [-0.0, 0.0, np.float32(1e-45)]                           # a -0, a +0 and the smallest subnormal
    I = BR.identity(dims)
    out, dx, _, _, tv, dg = _run_host(host_exe, x, d, I, dims, None, coef=10.0)
    assert np.array_equal(out, x) and same_bits(out + np.float32(0), x + np.float32(0))      # the bits, but for -0 -> +0
    assert out.reshape(-1)[0] == 0 and not np.signbit(out.reshape(-1)[0])
    nz = x != 0
    assert same_bits(out[nz], x[nz])
    assert np.array_equal(dx, d)                                                 # a flat grid has no guidance gradient
    assert tv == 0 and not dg.any()
    for w in _weights(W, H, dims)[1:]:
        out, dx, _, _, _, _ = _run_host(host_exe, x, d, I, dims, w)
        assert same_bits(out, w[None] * (x + np.float32(0)))                     # w * x exactly: masking a target needs no kernel of its own
        assert np.array_equal(out, w[None] * x)


def test_host_program_checks_itself_without_arguments(host_exe):
    """what _build/bilagrid_host_asan runs under ASan + UBSan: the built-in scene"""
    r = subprocess.run([host_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr


def test_cells_cover_the_grid_and_the_weights_are_a_partition():
    """the restatement against itself: every corner's vertex is inside the grid, a pixel
    beyond a luminance clamp sits on the first or last z vertex, and every term lands on exactly one vertex"""
    for shape in HOST_SHAPES:
        W, H, dims = shape[0], shape[1], shape[2:]
        x, d, G, w = BR.case(*shape, True, special=False)
        vertex, t = BR.terms(x, d, dims, w)
        assert vertex.min() >= 0 and vertex.max() < dims[0] * dims[1] * dims[2]
        _, _, (z0, z1, fz), l = BR.cells(x, dims)
        assert ((l <= 0) <= ((z0 == 0) & (fz == 0))).all() and ((l >= 1) <= (z1 == dims[2] - 1)).all()
        dG, A, n = BR.backward_grid(x, d, dims, w)
        assert n.sum() == 8 * W * H and np.all(A >= np.abs(dG))
        assert np.isclose(dG.sum(axis=0), t.reshape(-1, 12).sum(axis=0), rtol=1e-9, atol=1e-9).all()


# ---------------------------------------------------------------- the restatement against torch's grid_sample
def _nudged(shape, seed):
    """a case without the special samples whose luminance keeps 2^-10 from 0 and 1 (unless beyond them) and whose gz keeps 2^-10 from an integer:
    the float32 and the float64 z cells then agree"""
    x, d, G, w = BR.case(*shape, True, seed=seed, special=False)
    Gz, tol = shape[4], 2.0 ** -10
    for _ in range(64):
        l = 0.299 * x[0].astype(np.float64) + 0.587 * x[1] + 0.114 * x[2]
        gz = np.clip(l, 0, 1) * (Gz - 1)
        inside = (l > -tol) & (l < 1 + tol)
        bad = inside & (((np.abs(gz - np.round(gz)) < tol) & (Gz > 1)) | (np.abs(l) < tol) | (np.abs(l - 1) < tol))     # (Gz == 1: one z cell)
        if not bad.any():
            return x, d, G, w
        x[:, bad] += np.float32(2.0 ** -8)
    raise AssertionError("could not nudge the case")


def _torch_reference(x, d, G, dims, w):
    """(out, d_img, d_grid) of the grid_sample formulation in float64 with autograd"""
    import torch
    import torch.nn.functional as Fn
    Gx, Gy, Gz = dims
    _, H, W = x.shape
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Gt = torch.tensor(G, dtype=torch.float64, requires_grad=True)
    l = 0.299 * xt[0] + 0.587 * xt[1] + 0.114 * xt[2]
    cx = torch.arange(W, dtype=torch.float64) / (W - 1) if W > 1 else torch.zeros(1, dtype=torch.float64)
    cy = torch.arange(H, dtype=torch.float64) / (H - 1) if H > 1 else torch.zeros(1, dtype=torch.float64)
    coords = torch.stack([cx[None, :].expand(H, W), cy[:, None].expand(H, W), l.clamp(0, 1)], dim=-1) * 2 - 1     # (x, y, z) in [-1, 1]
    A = Fn.grid_sample(Gt.permute(3, 0, 1, 2)[None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    A = A.reshape(3, 4, H, W)
    out = (A[:, :3] * xt[None]).sum(1) + A[:, 3]
    if w is not None:
        out = out * torch.tensor(w, dtype=torch.float64)[None]
    (out * torch.tensor(d, dtype=torch.float64)).sum().backward()
    return out.detach().numpy(), xt.grad.numpy(), Gt.grad.numpy().reshape(-1, 12)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_against_torch_grid_sample_in_float64(shape, seed):
    dims = shape[2:]
    x, d, G, w = _nudged(shape, seed)
    out, d_img, d_grid = _torch_reference(x, d, G, dims, w)
    e_fwd = float(np.abs(BR.forward(x, G, dims, w) - out).max())                 # every pixel
    e_img = float(np.abs(BR.backward_image(x, d, G, dims, w) - d_img).max())
    dG, A, n = BR.backward_grid(x, d, dims, w)
    e_grid = float(np.abs(dG - d_grid).max() / np.abs(d_grid).max())             # every float of every vertex, relative to the largest
    print("twin against torch %s seed %d: forward %.3g  d_img %.3g  d_grid rel. max %.3g" % (shape, seed, e_fwd, e_img, e_grid))
    assert not np.abs(d_grid[n == 0]).any() and not dG[n == 0].any()             # untouched vertices: zero in both
    assert e_fwd <= FWD_BAR and e_img <= DIMG_BAR and e_grid <= DGRID_BAR


def test_total_variation_restatement_against_float64():
    for dims in ((4, 3, 2), (16, 16, 8), (3, 1, 4), (2, 5, 1), (1, 1, 1)):
        G = BR.case(8, 8, *dims, False)[2]
        g64 = G.astype(np.float64)
        want = sum(float((np.diff(g64, axis=ax) ** 2).mean()) for ax in (2, 1, 0) if G.shape[ax] >= 2)
        exact, most = BR.tv_exact(G)
        assert abs(exact - want) <= 1e-6 * max(want, 1e-30) and abs(float(BR.tv(G)) - exact) <= (most + 3) * 2.0 ** -53 * exact
        import torch
        Gt = torch.tensor(g64, requires_grad=True)
        sum(((Gt.diff(dim=ax)) ** 2).mean() for ax in (2, 1, 0) if G.shape[ax] >= 2).mul(10.0).backward() if want else None
        grad = BR.tv_grad(G, 10.0, np.zeros(G.size, np.float32))
        ref = Gt.grad.numpy() if want else np.zeros_like(g64)
        assert np.abs(grad - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max()))


# ---------------------------------------------------------------- the binding, appearance.BilateralGrid, train.trainStep: no GPU
def test_the_four_calls_are_in_the_binding():
    from gaussiansplat_amd import backend as B
    for name in ("gs_bilagrid_apply", "gs_bilagrid_backward", "gs_bilagrid_tv", "gs_bilagrid_adam"):
        assert name in B.ABI
        assert hasattr(B.Context, name[3:])
    assert B.GS_BILAGRID_FLOATS == 12 and B.GS_BILAGRID_MAX_DIM == 64


class _Stub:
    """what BilateralGrid reads of a renderer before it touches a device: the image's shape"""
    def __init__(self, H=4, W=5):
        self.imageData = np.zeros((3, H, W), np.float32)


def test_bilateral_grid_argument_checks_raise_before_any_gpu_call():
    from gaussiansplat_amd.appearance import BilateralGrid
    r = _Stub()
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            BilateralGrid(r, bad)
    for bad in ((16, 16), (0, 4, 4), (4, 65, 4), (4, 4, 1.5), "x", (4, 4, True)):
        with pytest.raises((ValueError, TypeError)):
            BilateralGrid(r, 2, grid=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            BilateralGrid(r, 2, lr=bad)
        with pytest.raises(ValueError):
            BilateralGrid(r, 2, tv_coef=bad)
    with pytest.raises(ValueError):
        BilateralGrid(r, 2, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        BilateralGrid(r, 2, eps=0.0)
    with pytest.raises(ValueError):
        BilateralGrid(r, 2, weights=[None])                                      # one entry per view
    with pytest.raises(ValueError):
        BilateralGrid(r, 2, weights=[None, np.zeros((5, 4), np.float32)])        # [W, H] is not [H, W]


def test_bilateral_grid_view_checks_on_a_host_tensor():
    """a torch CPU tensor stands in for imageData: the object is built, and a view out of range is refused before any call into the library"""
    import torch
    from gaussiansplat_amd import train as TR
    from gaussiansplat_amd.appearance import BilateralGrid, Exposure

    class R:
        imageData = torch.zeros((3, 4, 5))
    b = BilateralGrid(R(), 3, grid=(4, 3, 2), weights=[None, np.ones((4, 5), np.float32), None])
    assert tuple(b.table.shape) == (3, 2, 3, 4, 12) and b.dims == (4, 3, 2) and b.step_counts == [0, 0, 0]
    assert np.array_equal(b.grid(2), BR.identity((4, 3, 2))) and b.lr == 2e-3 and b.tv_coef == 10.0
    for bad in (-1, 3, 1.5, None, True):
        for call in (lambda: b.apply(bad, R.imageData), lambda: b.backward(bad, R.imageData), lambda: b.step(bad),
                     lambda: b.mask_target(bad, R.imageData), lambda: b.grid(bad), lambda: b.tv(bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        b.apply(0, torch.zeros((3, 5, 4)))
    with pytest.raises(ValueError):
        b.backward(0, R.imageData)                                               # no apply before it
    with pytest.raises(ValueError):
        b.set_lr(-1.0)
    gt = torch.zeros((3, 4, 5))
    assert b.mask_target(0, gt) is gt                                            # no weight: the target itself
    sd = b.state_dict()
    assert set(sd) == {"table", "exp_avg", "exp_avg_sq", "steps", "lr"} and sd["lr"] == 2e-3
    sd["steps"] = [4, 0, 2]; sd["lr"] = 0.005
    b.load_state_dict(sd)
    assert b.step_counts == [4, 0, 2] and b.lr == 0.005
    with pytest.raises(ValueError):
        b.load_state_dict(dict(sd, steps=[1, 2]))
    with pytest.raises(ValueError):
        b.load_state_dict(dict(sd, table=torch.zeros((3, 2, 3, 4, 11))))
    # trainStep: the pair goes together, grid and exposure are alternatives, and the view is checked before anything is rendered
    e = Exposure(R(), 3)
    with pytest.raises(ValueError):
        TR.trainStep(None, gt, 0.1, None, bilagrid=b)
    with pytest.raises(ValueError):
        TR.trainStep(None, gt, 0.1, None, bilagrid=b, view=3)
    with pytest.raises(ValueError, match="alternatives"):
        TR.trainStep(None, gt, 0.1, None, bilagrid=b, exposure=e, view=0)
    with pytest.raises(ValueError):
        TR.trainStep(None, gt, 0.1, None, view=0)
