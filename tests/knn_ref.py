"""The reference of gs_knn_mean_dist2 (include/gsplat.h): NumPy float32 brute force in row chunks, and the clouds the tests run.

d2 = ((dx*dx + dy*dy) + dz*dz) on float32 arrays -- every operation one fp32 operation, as the contract says -- with the diagonal set to
+Inf, rows that are not finite removed, the three smallest values of a row taken by `partition`, dist2 = ((b0 + b1) + b2) / float32(3).
The result is a function of a multiset of individually rounded values, so any exact search equals it bit for bit.
"""
import numpy as np

from common import same_bits

NAN, INF = np.float32("nan"), np.float32("inf")
BOX = 64                                   # GS_KNN_BOX (tests/test_pointcloud_host.py checks it against csrc/gs_knn.h and backend.KNN_BOX)


def knn_mean_dist2(points, chunk=512):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = p.shape[0]
    out = np.full(n, NAN, np.float32)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    if len(fin) < 4:
        return out
    q = p[fin]
    m = q.shape[0]
    res = np.empty(m, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, m, chunk):
            hi = min(m, lo + chunk)
            dx = q[lo:hi, None, 0] - q[None, :, 0]
            dy = q[lo:hi, None, 1] - q[None, :, 1]
            dz = q[lo:hi, None, 2] - q[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[np.arange(hi - lo), np.arange(lo, hi)] = INF
            b = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
            res[lo:hi] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3)
    out[fin] = res
    return out


def torch_brute(points, chunk=1024):
    """The same brute force in torch on the points' device (finite points only): chunked rows, separate sub / mul / add -- eager torch
    rounds every one on its own -- and no cdist.  An independent yardstick for larger clouds, and for the time of tools/knn_time.py.
    The last step, / 3, is done in NumPy on the host: torch turns a division by a scalar into a multiplication by its reciprocal."""
    import torch
    n = points.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=points.device)
    x, y, z = (points[:, a].contiguous() for a in range(3))
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=points.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        dx = torch.sub(x[lo:hi, None], x[None, :])
        dy = torch.sub(y[lo:hi, None], y[None, :])
        dz = torch.sub(z[lo:hi, None], z[None, :])
        d2 = torch.add(torch.add(torch.mul(dx, dx), torch.mul(dy, dy)), torch.mul(dz, dz))
        rows = torch.arange(hi - lo, device=points.device)
        d2[rows, rows + lo] = inf
        b = torch.topk(d2, 3, dim=1, largest=False, sorted=True).values
        out[lo:hi] = torch.add(torch.add(b[:, 0], b[:, 1]), b[:, 2])
    return out.cpu().numpy() / np.float32(3)


# ---------------------------------------------------------------- the clouds
def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def clustered(n_blob=1000, n_out=100, seed=2):
    """three blobs of sigma 1e-3 and outliers at scale 1e4"""
    rng = np.random.default_rng(seed)
    centres = rng.random((3, 3)).astype(np.float32)
    blobs = [c + np.float32(1e-3) * rng.standard_normal((n_blob, 3)).astype(np.float32) for c in centres]
    return np.concatenate(blobs + [np.float32(1e4) * rng.standard_normal((n_out, 3)).astype(np.float32)]).astype(np.float32)


DUP_GROUPS = ((10, 2), (20, 3), (30, 4), (40, 5))          # (first row, size) of the planted groups of identical points


def duplicates(n=1000, seed=3):
    p = uniform(n, seed)
    for first, size in DUP_GROUPS:
        p[first:first + size] = p[first]
    return p


def all_identical(n=1500):
    return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (n, 1))


def on_a_line(n=777, seed=4):
    t = np.random.default_rng(seed).random(n, dtype=np.float32)
    return np.stack([t, np.full(n, 2.0, np.float32), np.full(n, -1.0, np.float32)], axis=1)


def on_a_plane(n=1300, seed=5):
    p = uniform(n, seed)
    p[:, 1] = np.float32(0.5)
    return p


def lattice(k=16):
    g = np.arange(k, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def lattice_interior(k=16):
    g = np.arange(k)
    i = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return ((i > 0) & (i < k - 1)).all(axis=1)


NONFINITE_ROWS = (0, 1, 5, 64, 100, 511, 1000, 1001, 1500, 1998, 1999, 777)


def nonfinite(n=2000, seed=6):
    p = uniform(n, seed)
    vals = (NAN, INF, -INF)
    for k, r in enumerate(NONFINITE_ROWS):
        p[r, k % 3] = vals[(k // 3) % 3]
    return p


def too_few():
    p = uniform(6, 7)
    p[0, 0], p[2, 1], p[5, 2] = NAN, INF, -INF
    return p


def overflow(n=16, seed=8):
    """sparse enough that every squared distance overflows (neighbours ~0.3e20 apart, squares beyond 3.4e38)"""
    return uniform(n, seed) * np.float32(1e20)


def overflow_mixed(n=500, seed=8):
    """denser: some of the three smallest squares overflow and some do not -- +Inf takes part in the triple as a value"""
    return uniform(n, seed) * np.float32(1e20)


def clouds():
    """name -> points; every one is small enough for the CPU pipeline (n <= 4 097)"""
    out = {f"uniform{n}": uniform(n, 100 + n) for n in (4, 5, 63, 64, 65, BOX - 1, BOX, BOX + 1, 4097)}
    out.update(clustered=clustered(), duplicates=duplicates(), all_identical=all_identical(), line=on_a_line(), plane=on_a_plane(),
               lattice=lattice(), nonfinite=nonfinite(), too_few=too_few(), overflow=overflow(), overflow_mixed=overflow_mixed())
    return out


def check_planted(name, pts, ref):
    """Each planted case, on the REFERENCE's output alone, gives its kind of result."""
    if name == "duplicates":
        for first, size in DUP_GROUPS:
            grp = ref[first:first + size]
            assert np.all(grp == 0.0) if size >= 4 else np.all(grp > 0.0), (first, size, grp)
    elif name == "all_identical":
        assert np.all(ref == 0.0)
    elif name == "lattice":
        assert np.all(ref[lattice_interior()] == 1.0)
    elif name == "nonfinite":
        rows = np.array(NONFINITE_ROWS)
        keep = np.setdiff1d(np.arange(len(pts)), rows)
        assert np.isnan(ref[rows]).all() and np.isfinite(ref[keep]).all()
        assert same_bits(ref[keep], knn_mean_dist2(pts[keep]), nan_equal=True)
    elif name == "too_few":
        assert np.isnan(ref).all()
    elif name == "overflow":
        assert np.all(ref == INF)
    elif name == "overflow_mixed":
        assert np.count_nonzero(ref == INF) >= 50 and np.count_nonzero(np.isfinite(ref)) >= 50 and not np.isnan(ref).any()
    else:
        assert np.isfinite(ref).all() and np.all(ref >= 0.0)
