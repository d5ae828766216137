"""NumPy restatement of the per-view bilateral grid (csrc/gs_bilagrid.h; include/gsplat.h: gs_bilagrid_apply / _backward / _tv).

Images are planar [3, H, W] float32, the grid G is [Gz, Gy, Gx, 12] float32 (12 = A[r][k], row-major 3 x 4), the weight [H, W] float32 or
None; dims = (Gx, Gy, Gz).  Everything float32 is float32 operation by operation, in the header's order (NumPy has no fma contraction):
    cell      g = g < n - 1 ? g : n - 1;  i0 = min((int)g, max(n - 2, 0));  i1 = min(i0 + 1, n - 1);  f = g - i0
    pixel     gx = c sx, sx = float32((Gx - 1) / (W - 1)) (0 when W == 1), gy likewise;  l = (0.299 x0 + 0.587 x1) + 0.114 x2;
              lc = l > 0 ? l : 0;  lc = lc < 1 ? lc : 1;  gz = lc (Gz - 1)
    slice     e[z][y] = G[z][y][x0] + fx (G[z][y][x1] - G[z][y][x0]);  h[z] = e[z][y0] + fy (e[z][y1] - e[z][y0]);  S = h[z1] - h[z0];  A = h[z0] + fz S
    forward   a_r = ((A[r][0] x0 + A[r][1] x1) + A[r][2] x2) + A[r][3];  out_r = w a_r  (no weight: a_r)
    into x    g_r = w d_r (no weight: d_r);  dA[r][k] = g_r x_k (k = 3: g_r);  dl = (Gz - 1) (((dA[0] S[0] + dA[1] S[1]) + ...) + dA[11] S[11]) when
              0 < l < 1, else 0;  dx_k = ((A[0][k] g0 + A[1][k] g1) + A[2][k] g2) + lam_k dl,  lam = (0.299, 0.587, 0.114)
    into G    u = (wz wy) wx per corner (w?0 = 1 - f?, w?1 = f?), corners z0y0x0, z0y0x1, z0y1x0, ...;  the term of a corner into float [r][k] of its
              vertex is float64(u) * (float64(g_r) * float64(x_k)): the inner product exact, the outer rounded once.  d_grid[v][m] is EXACT here:
              math.fsum of the terms of every (pixel, corner) whose vertex is v; A_v = fsum of their magnitudes, n_v the number of terms.
    TV        per axis with n >= 2: S = sum of float64(d)^2, d = G[+1] - G in float32; tv = (S_x / count_x + S_y / count_y) + S_z / count_z.  tv()
              adds the squares one after another in the order of the grid's floats (what tests/bilagrid_host.cpp does: bit for bit); tv_exact()
              is fsum.  tv_grad: acc = d_grid; per axis x, y, z: acc = acc + s (G - G[-1]) where there is a vertex before, acc = acc - s (G[+1] - G)
              where there is one behind; s = float32(2 coef / count)."""
import math

import numpy as np

F = np.float32
# (W, H, Gx, Gy, Gz): odd pixel count and the 4-byte path with a tail; the default grid on the 16-byte path; an image smaller than the grid; two
# degenerate axes each way (no guidance gradient at Gz == 1); several workgroups and partial rows per vertex
SHAPES = [(37, 23, 4, 3, 2), (80, 56, 16, 16, 8), (5, 3, 16, 16, 8), (64, 1, 3, 1, 4), (1, 9, 2, 5, 1), (300, 200, 16, 16, 8)]
LAM = (F(0.299), F(0.587), F(0.114))


def identity(dims):
    Gx, Gy, Gz = dims
    return np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (Gz, Gy, Gx, 1))


def scale(n, extent):
    return F((n - 1) / (extent - 1)) if extent > 1 else F(0)


def cell(g, n):
    """(i0, i1, f) of float32 coordinates g on an axis of n vertices"""
    g = np.asarray(g, F)
    top = F(n - 1)
    g = np.where(g < top, g, top)
    i0 = np.minimum(g.astype(np.int32), max(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, g - i0.astype(F)


def luminance(x):
    return (F(0.299) * x[0] + F(0.587) * x[1]) + F(0.114) * x[2]


def cells(x, dims):
    """the cells of every pixel: x [W], y [H] and z [H, W] triples (i0, i1, f), and the luminance [H, W]"""
    Gx, Gy, Gz = dims
    _, H, W = x.shape
    with np.errstate(invalid="ignore"):
        l = luminance(x)
        lc = np.where(l > 0, l, F(0))
        lc = np.where(lc < 1, lc, F(1))
    cx = cell(np.arange(W).astype(F) * scale(Gx, W), Gx)
    cy = cell(np.arange(H).astype(F) * scale(Gy, H), Gy)
    cz = cell(lc * F(Gz - 1), Gz)
    return cx, cy, cz, l


def slice_grid(G, c):
    """(A, S): [H, W, 12] float32 each"""
    (x0, x1, fx), (y0, y1, fy), (z0, z1, fz), _ = c
    xs, ys, zs = (x0[None, :], x1[None, :]), (y0[:, None], y1[:, None]), (z0, z1)
    fx, fy, fz = fx[None, :, None], fy[:, None, None], fz[:, :, None]
    h = []
    with np.errstate(invalid="ignore", over="ignore"):
        for z in zs:
            e = []
            for y in ys:
                g0, g1 = G[z, y, xs[0]], G[z, y, xs[1]]
                e.append(g0 + fx * (g1 - g0))
            h.append(e[0] + fy * (e[1] - e[0]))
        S = h[1] - h[0]
        return h[0] + fz * S, S


def weigh(d, w=None):
    d = np.asarray(d, F)
    return d.copy() if w is None else (np.asarray(w, F)[None] * d).astype(F)


def forward(x, G, dims, w=None):
    x, G = np.asarray(x, F), np.asarray(G, F)
    A, _ = slice_grid(G, cells(x, dims))
    out = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            a = ((A[..., 4 * r] * x[0] + A[..., 4 * r + 1] * x[1]) + A[..., 4 * r + 2] * x[2]) + A[..., 4 * r + 3]
            out[r] = a if w is None else np.asarray(w, F) * a
    return out


def backward_image(x, d, G, dims, w=None):
    x, G = np.asarray(x, F), np.asarray(G, F)
    c = cells(x, dims)
    A, S = slice_grid(G, c)
    l, g = c[3], weigh(d, w)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = None
        for r in range(3):
            for k in range(4):
                dA = g[r] * x[k] if k < 3 else g[r]
                t = dA * S[..., 4 * r + k]
                acc = t if acc is None else acc + t
        dl = np.where((0 < l) & (l < 1), F(dims[2] - 1) * acc, F(0))
        dx = np.empty_like(x)
        for k in range(3):
            dx[k] = ((A[..., k] * g[0] + A[..., 4 + k] * g[1]) + A[..., 8 + k] * g[2]) + LAM[k] * dl
    return dx


def terms(x, d, dims, w=None):
    """(vertex, t): [8, H W] int32 and [8, H W, 12] float64 -- the vertex of every corner of every pixel and its twelve exact-product terms"""
    x = np.asarray(x, F)
    Gx, Gy, Gz = dims
    _, H, W = x.shape
    (x0, x1, fx), (y0, y1, fy), (z0, z1, fz), _ = cells(x, dims)
    g = weigh(d, w).astype(np.float64).reshape(3, -1)
    xa = np.concatenate([x.astype(np.float64).reshape(3, -1), np.ones((1, H * W))], axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        gx = (g[:, None, :] * xa[None, :, :]).reshape(12, -1).T                    # [P, 12], exact
        wx, wy, wz = (F(1) - fx, fx), (F(1) - fy, fy), (F(1) - fz, fz)
        vertex, t = np.empty((8, H * W), np.int32), np.empty((8, H * W, 12), np.float64)
        for k in range(8):
            zi, yi, xi = (k >> 2) & 1, (k >> 1) & 1, k & 1
            u = (wz[zi] * wy[yi][:, None]) * wx[xi][None, :]
            assert u.dtype == F
            vertex[k] = (((z1 if zi else z0) * Gy + (y1 if yi else y0)[:, None]) * Gx + (x1 if xi else x0)[None, :]).reshape(-1)
            t[k] = u.astype(np.float64).reshape(-1, 1) * gx
    return vertex, t


def backward_grid(x, d, dims, w=None):
    """(d_grid, A, n): [Gz Gy Gx, 12] float64 the correctly rounded sums of the terms and of their magnitudes, and [Gz Gy Gx] the number of
    terms of each vertex"""
    Gx, Gy, Gz = dims
    nv = Gx * Gy * Gz
    vertex, t = terms(x, d, dims, w)
    vertex, t = vertex.reshape(-1), t.reshape(-1, 12)
    order = np.argsort(vertex, kind="stable")
    vertex, t = vertex[order], t[order]
    n = np.bincount(vertex, minlength=nv)
    start = np.concatenate([[0], np.cumsum(n)])
    dG, A = np.zeros((nv, 12), np.float64), np.zeros((nv, 12), np.float64)
    for v in np.nonzero(n)[0]:
        cols = t[start[v]:start[v + 1]].T.tolist()
        for m in range(12):
            dG[v, m] = math.fsum(cols[m])                                         # (a NaN term gives NaN)
            A[v, m] = math.fsum(abs(c) for c in cols[m])
    return dG, A, n


def terms_per_pixel(dims):
    """the corners of one pixel that fall on the same vertex: 2 per axis of one vertex"""
    return 2 ** sum(1 for n in dims if n == 1)


def dG_bound(dG, A, n):
    """|device - exact| <= n 2^-53 A + 2^-24 |exact| + 2^-149 per entry, n the number of terms of the vertex: any order of summing n terms in double
    ((n - 1) u A, u = 2^-53; lanes without a term add + 0, which is exact), then the one rounding to float.  n = c n_v with n_v the pixels
    touching the vertex and c = terms_per_pixel(dims)."""
    return n[:, None] * 2.0 ** -53 * A + 2.0 ** -24 * np.abs(dG) + 2.0 ** -149


# ---------------------------------------------------------------- total variation
def _axes(G):
    """(axis of G, count) in the order x, y, z for the axes with two vertices or more"""
    return [(ax, (G.shape[ax] - 1) * (G.size // G.shape[ax])) for ax in (2, 1, 0) if G.shape[ax] >= 2]


def _sq(G, ax):
    """float64(d)^2 of the forward differences along ax, in the order of the floats they start from"""
    d = np.diff(np.asarray(G, F), axis=ax)
    assert d.dtype == F
    return (d.astype(np.float64) ** 2).reshape(-1)


def tv(G):
    out = None
    for ax, count in _axes(G):
        sq = _sq(G, ax)
        q = (np.cumsum(sq)[-1] if sq.size else 0.0) / count                     # cumsum adds one after another
        out = q if out is None else out + q
    return np.float64(0.0 if out is None else out)


def tv_exact(G):
    """(tv with every sum correctly rounded, the largest number of squares in one sum)"""
    parts = [(math.fsum(_sq(G, ax).tolist()) / count, count) for ax, count in _axes(G)]
    return sum(p for p, _ in parts), max([c for _, c in parts], default=0)


def tv_grad(G, coef, d_grid):
    G = np.asarray(G, F)
    acc = np.array(d_grid, F).reshape(G.shape)
    for ax, count in _axes(G):
        s = F(2.0 * float(F(coef)) / count)
        d = np.diff(G, axis=ax)                                                   # G[+1] - G
        back, fwd = [slice(None)] * 4, [slice(None)] * 4
        back[ax], fwd[ax] = slice(1, None), slice(0, -1)
        acc[tuple(back)] = acc[tuple(back)] + s * d                               # (i > 0)      acc + s (G - G[-1])
        acc[tuple(fwd)] = acc[tuple(fwd)] - s * d                                 # (i < n - 1)  acc - s (G[+1] - G)
    return acc


# ---------------------------------------------------------------- cases
def case(W, H, Gx, Gy, Gz, weighted, seed=0, special=True):
    """x ~ U(-0.1, 1.1) (1-2 % of the luminances beyond each clamp), d ~ N(0, 1), G = identity + N(0, 0.2^2), w uniform in [0, 1] with a
    quarter of the pixels exactly 0 and an eighth exactly 1.  special: pixel 0 is -0 in every channel (l = -0) and one channel of the middle
    pixel is NaN."""
    rng = np.random.default_rng(100003 * W + 1009 * H + 101 * Gx + 11 * Gy + Gz + 7 * seed)
    x = (rng.random((3, H, W)) * 1.2 - 0.1).astype(F)
    d = rng.standard_normal((3, H, W)).astype(F)
    G = (identity((Gx, Gy, Gz)) + 0.2 * rng.standard_normal((Gz, Gy, Gx, 12))).astype(F)
    w = None
    if weighted:
        w = rng.random((H, W), dtype=F)
        perm = rng.permutation(W * H)
        w.reshape(-1)[perm[:(W * H + 2) // 4]] = 0.0
        w.reshape(-1)[perm[(W * H + 2) // 4:(W * H + 2) // 4 + (W * H + 4) // 8]] = 1.0
    if special:
        x[:, 0, 0] = -0.0
        x[1, H // 2, W // 2] = np.nan
    return x, d, G, w
