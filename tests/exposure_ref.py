"""NumPy restatement of the per-view exposure stage (csrc/gs_exposure.h; include/gsplat.h: gs_exposure_apply / gs_exposure_backward).

Images are planar [3, H, W] float32, E is [3, 4] float32 (row r: the matrix row, then the offset), the weight [H, W] float32 or None.
The forward and the adjoint into the image are float32, operation by operation (NumPy has no fma contraction):
    a_r = ((E[r][0] x0 + E[r][1] x1) + E[r][2] x2) + E[r][3];   out_r = w a_r   (no weight: a_r)
    g_r = w d_r   (no weight: d_r);   dx_k = (E[0][k] g0 + E[1][k] g1) + E[2][k] g2
The adjoint into E is EXACT: t[r][k] = float64(g_r) * float64(x_k) (x_3 = 1) is exact in double, and dE[r][k] = math.fsum of the terms, the
correctly rounded sum.  A[r][k] = fsum |t[r][k]| is kept beside it: what bounds the error of any order of summing the terms in double."""
import math

import numpy as np

SHAPES = [(1, 1), (3, 1), (5, 7), (64, 1), (67, 3), (256, 4), (129, 33), (320, 200)]      # (W, H)


def forward(x, E, w=None):
    x, E = np.asarray(x, np.float32), np.asarray(E, np.float32).reshape(3, 4)
    out = np.empty_like(x)
    for r in range(3):
        a = ((E[r, 0] * x[0] + E[r, 1] * x[1]) + E[r, 2] * x[2]) + E[r, 3]
        out[r] = a if w is None else np.asarray(w, np.float32) * a
    return out


def weigh(d, w=None):
    d = np.asarray(d, np.float32)
    return d.copy() if w is None else (np.asarray(w, np.float32)[None] * d).astype(np.float32)


def backward_image(d, E, w=None):
    g, E = weigh(d, w), np.asarray(E, np.float32).reshape(3, 4)
    dx = np.empty_like(g)
    for k in range(3):
        dx[k] = (E[0, k] * g[0] + E[1, k] * g[1]) + E[2, k] * g[2]
    return dx


def terms(x, d, w=None):
    """[3, 4, P] float64: the exact per-pixel terms of the adjoint into E."""
    g = weigh(d, w).astype(np.float64).reshape(3, -1)
    x = np.asarray(x, np.float32).astype(np.float64).reshape(3, -1)
    xa = np.concatenate([x, np.ones((1, x.shape[1]))], axis=0)
    return g[:, None, :] * xa[None, :, :]


def backward_exposure(x, d, w=None):
    """(dE, A): [3, 4] float64 each, the correctly rounded sums of the terms and of their magnitudes."""
    t = terms(x, d, w)
    dE = np.array([[math.fsum(t[r, k]) for k in range(4)] for r in range(3)], np.float64)
    A = np.array([[math.fsum(np.abs(t[r, k])) for k in range(4)] for r in range(3)], np.float64)
    return dE, A


def dE_bound(dE, A, P):
    """|device - exact| <= P 2^-53 A + 2^-24 |exact| + 2^-149 per entry: any order of summing P exact terms in double ((P - 1) u A, u = 2^-53),
    then the one rounding to float (normal: 2^-24 relative; subnormal: half the smallest step)."""
    return P * 2.0 ** -53 * A + 2.0 ** -24 * np.abs(dE) + 2.0 ** -149


def identity():
    return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def case(W, H, weighted, seed=0):
    """The inputs of a test case: x, d ~ N(0, 1), E = [I | 0] + N(0, 0.2^2), w uniform in [0, 1] with a quarter of the pixels exactly 0."""
    rng = np.random.default_rng(1000 * W + H + 7 * seed)
    x = rng.standard_normal((3, H, W)).astype(np.float32)
    d = rng.standard_normal((3, H, W)).astype(np.float32)
    E = (identity() + 0.2 * rng.standard_normal((3, 4))).astype(np.float32)
    w = None
    if weighted:
        w = rng.random((H, W), dtype=np.float32)
        w.reshape(-1)[rng.permutation(W * H)[:(W * H + 2) // 4]] = 0.0
    return x, d, E, w
