"""The per-gaussian statements of the numeric spec (csrc/gs_pergaussian.h, csrc/gs_detmath.h) on the CPU, against the oracle, bit for bit.

The statements that decide tile ids and depth keys are __host__ __device__ functions: tests/pergaussian_host.cpp is a host build of them
(contraction off), run as a child process on the oracle's own cov2d and mu.  Equality is of bit patterns, NaN matching NaN, no tolerance:
every operation is individually rounded on both sides.  So that nothing passes on empty work, the oracle's output alone must show that at
least a quarter of the rectangles are non-empty and that every planted row is there and gives its kind of result."""
import ctypes as C

import numpy as np
import pytest

from common import bits, host_program, run_host, same_bits, scene_and_cameras
from gaussiansplat_amd import synthetic

N3, W3, H3, SEED3 = 4096, 400, 300, 31
N2, W2, H2, SEED2 = 1024, 200, 150, 32
NAN, INF = np.float32("nan"), np.float32("inf")
# planted rows of the 3-D set ...
NAN_MEAN, INF_SCALE, SCALE_90, TZ_ZERO, SINGULAR, OFF_SCREEN, LEFT, RIGHT, TOP, BOTTOM = range(10)
# ... and of the 2-D set (no depth, and + 0.3 I keeps its covariance regular)
NAN_MEAN2, INF_SCALE2, SCALE_90_2, OFF_SCREEN2, LEFT2, RIGHT2, TOP2, BOTTOM2 = range(8)


def oracle_rects(O, bbs, gx, gy):
    out = np.zeros((bbs.shape[0], 4), np.int32)                     # 0 0 0 0 where the oracle returns 0
    rc = (C.c_int32 * 4)()
    for g in range(bbs.shape[0]):
        bb = np.ascontiguousarray(bbs[g], np.float32)
        if O.lib().gso_tile_rect(bb.ctypes.data_as(C.POINTER(C.c_float)), 16, gx, gy, rc):
            out[g] = tuple(rc)
    return out


def edge_means(O, sc, ocam, deg):
    """Means (z = 0) whose projected centre is nearest each image edge: found with the oracle on a line of candidates."""
    k = 4001
    line = {key: np.repeat(v[:1], 2 * k, axis=0) for key, v in sc.items()}
    line["means"] = np.zeros((2 * k, 3), np.float32)
    line["means"][:k, 0] = np.linspace(-12.0, 12.0, k)
    line["means"][k:, 1] = np.linspace(-12.0, 12.0, k)
    mu = O.preprocess(line["means"], line["scales"], line["quats"], line["opacities"], line["shs"], deg, ocam)["mu"]
    pick = lambda lo, hi, c, target: line["means"][lo + int(np.argmin(np.abs(mu[lo:hi, c] - target)))]
    return pick(0, k, 0, 0.5), pick(0, k, 0, W3 + 0.5), pick(k, 2 * k, 1, 0.5), pick(k, 2 * k, 1, H3 + 0.5)


@pytest.fixture(scope="module")
def sets(oracle):
    O = oracle
    deg = 1
    sc, cam, T, P, ocam = scene_and_cameras(N3, W3, H3, deg, SEED3)
    sc["scales"][:10] = -3.0                                             # the planted rows: small splats unless the row says otherwise
    sc["means"][:10] = 0.0
    sc["means"][NAN_MEAN, 1] = NAN
    sc["scales"][INF_SCALE, 0] = INF
    sc["scales"][SCALE_90, 2] = 90.0                                     # exp overflows
    sc["means"][TZ_ZERO] = cam.eye                                       # t = T [eye; 1] = 0 exactly (compute_transform's own sums, negated)
    sc["scales"][SINGULAR] = -100.0                                      # exp underflows to 0: cov2d = 0.3 in all four entries
    sc["means"][OFF_SCREEN, 0] = 40.0
    for row, m in zip((LEFT, RIGHT, TOP, BOTTOM), edge_means(O, sc, ocam, deg)):
        sc["means"][row] = m
        sc["scales"][row] = -1.5
    pre3 = O.preprocess(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], deg, ocam)
    s2 = synthetic.make_scene_2d(N2, W2, H2, SEED2)
    s2["means"][:8] = 0.5
    s2["scales"][:8] = 1.0
    s2["means"][NAN_MEAN2, 0] = NAN
    s2["scales"][INF_SCALE2, 1] = INF
    s2["scales"][SCALE_90_2, 0] = 90.0
    s2["means"][OFF_SCREEN2] = (5.0, -3.0)
    s2["means"][LEFT2, 0], s2["means"][RIGHT2, 0], s2["means"][TOP2, 1], s2["means"][BOTTOM2, 1] = 0.0, 1.0, 0.0, 1.0
    pre2 = O.preprocess2d(s2["means"], s2["scales"], s2["rots"], s2["opacities"], s2["colors"], W2, H2)
    for pre, W, H in ((pre3, W3, H3), (pre2, W2, H2)):
        pre["rect"] = oracle_rects(O, pre["bbs"], (W + 15) // 16, (H + 15) // 16)
    rng = np.random.default_rng(33)
    z = np.concatenate([pre3["tps"][:, 2], np.array([NAN, INF, -INF, 0.0, -0.0], np.float32)])
    x = rng.uniform(-100.0, 100.0, 4096).astype(np.float32)
    hi, lo = np.float32(88.72283), np.float32(-87.33654)                 # gs_expf's thresholds, and the floats beside them
    x[:11] = [NAN, INF, -INF, hi, np.nextafter(hi, INF), np.nextafter(hi, -INF), lo, np.nextafter(lo, -INF), np.nextafter(lo, INF), 0.0, -0.0]
    ang = rng.uniform(-10.0, 10.0, 4096).astype(np.float32)
    ang[:8] = [INF, -INF, NAN, 0.0, -0.0, 1.0e5, -3.0e7, np.float32(np.pi / 4)]
    quats = np.concatenate([sc["quats"][:2048], rng.standard_normal((2048, 4)).astype(np.float32)])
    words = rng.integers(-2 ** 62, 2 ** 62, 4096, dtype=np.int64)
    words[:4] = [0, -1, 2 ** 62, -2 ** 62]
    comp = rng.integers(0, 10, 4096).astype(np.int32)
    return dict(O=O, sc=sc, pre3=pre3, s2=s2, pre2=pre2, z=z, x=x, ang=ang, quats=quats, words=words, comp=comp)


@pytest.fixture(scope="module")
def host(sets, tmp_path_factory):
    """What the host build of the header computes from the oracle's cov2d and mu and from the raw inputs"""
    exe = host_program("pergaussian", tmp_path_factory.mktemp("pergaussian_host"))
    s = sets
    nz, nx, na, nq, nf = len(s["z"]), len(s["x"]), len(s["ang"]), len(s["quats"]), len(s["words"])
    fixed = np.empty((nf, 3), np.uint32)
    fixed[:, 0] = (s["words"].view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    fixed[:, 1] = (s["words"].view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    fixed[:, 2] = s["comp"].view(np.uint32)
    arrays = [np.asarray(a, np.float32) for a in (s["pre3"]["cov2d"], s["pre3"]["mu"], s["pre2"]["cov2d"], s["pre2"]["mu"], s["z"], s["x"], s["ang"], s["quats"])]
    layout = (("invcov3", (N3, 4)), ("bbs3", (N3, 4)), ("rect3", (N3, 4)), ("invcov2", (N2, 4)), ("bbs2", (N2, 4)), ("rect2", (N2, 4)), ("keys", (3, nz)),
              ("exp", (nx,)), ("sin", (na,)), ("cos", (na,)), ("R", (nq, 3, 3)), ("fixed", (nf,)))
    dtype = lambda key: np.uint32 if key == "keys" else np.int32 if key.startswith("rect") else np.float32
    res = run_host(exe, [], np.array([N3, W3, H3, N2, W2, H2, nz, nx, na, nq, nf], np.uint32).tobytes(), arrays + [fixed],
                   [(dtype(key), int(np.prod(shape))) for key, shape in layout])
    return {key: a.reshape(shape) for (key, shape), a in zip(layout, res)}


def test_the_oracle_output_is_real_work(sets):
    p3, p2 = sets["pre3"], sets["pre2"]
    for pre, n in ((p3, N3), (p2, N2)):
        assert np.count_nonzero(pre["rect"][:, 0]) >= n // 4
    empty = lambda pre, g: not pre["rect"][g].any()
    nan_box = lambda pre, g: bool(np.isnan(pre["bbs"][g]).any()) and empty(pre, g)
    assert nan_box(p3, NAN_MEAN) and nan_box(p3, INF_SCALE) and nan_box(p3, SCALE_90) and nan_box(p3, TZ_ZERO)
    assert p3["ts"][TZ_ZERO, 2] == 0.0
    assert np.all(bits(p3["cov2d"][SINGULAR]) == bits(p3["cov2d"][SINGULAR])[0]) and not np.isfinite(p3["invcov"][SINGULAR]).any()
    assert np.isfinite(p3["bbs"][OFF_SCREEN]).all() and empty(p3, OFF_SCREEN)
    assert nan_box(p2, NAN_MEAN2) and nan_box(p2, INF_SCALE2) and nan_box(p2, SCALE_90_2)
    assert np.isfinite(p2["bbs"][OFF_SCREEN2]).all() and empty(p2, OFF_SCREEN2)
    # a straddler: its centre within a pixel of the edge, its box cut there (bbs = xmin ymin xmax ymax), its rectangle not empty
    for pre, rows, W, H in ((p3, (LEFT, RIGHT, TOP, BOTTOM), W3, H3), (p2, (LEFT2, RIGHT2, TOP2, BOTTOM2), W2, H2)):
        for g, c, at, edge in zip(rows, (0, 2, 1, 3), (0.0, float(W), 0.0, float(H)), (1.0, float(W), 1.0, float(H))):
            assert abs(pre["mu"][g, c % 2] - at) <= 1.0 and pre["bbs"][g, c] == edge and pre["rect"][g, 0] > 0, (g, pre["mu"][g], pre["bbs"][g])


def test_conic_box_and_tile_rectangle(sets, host):
    for tag in ("3", "2"):
        pre = sets["pre" + tag]
        assert same_bits(host["invcov" + tag], pre["invcov"], nan_equal=True)
        assert same_bits(host["bbs" + tag], pre["bbs"], nan_equal=True)
        assert np.array_equal(host["rect" + tag], pre["rect"])


def test_depth_keys(sets, host):
    O = sets["O"]
    for order in (O.ORDER_INDEX, O.ORDER_DEPTH_DESC, O.ORDER_DEPTH_ASC):
        want = np.array([O.lib().gso_depth_key(C.c_float(float(v)), order) for v in sets["z"]], np.uint32)
        assert np.array_equal(host["keys"][order], want)


def test_exp_and_sincos(sets, host):
    O = sets["O"]
    assert same_bits(host["exp"], np.array([O.expf(float(v)) for v in sets["x"]], np.float32), nan_equal=True)
    sc = np.array([O.sincosf(float(v)) for v in sets["ang"]], np.float32)
    assert same_bits(host["sin"], sc[:, 0], nan_equal=True) and same_bits(host["cos"], sc[:, 1], nan_equal=True)


def test_quat_to_rot(sets, host):
    w, x, y, z = (sets["quats"][:, i] for i in range(4))                # float32 arrays: every operation below is one fp32 operation
    one, two = np.float32(1.0), np.float32(2.0)
    R = np.empty((len(w), 3, 3), np.float32)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 1, 0] = two * (x * y + w * z)
    R[:, 2, 0] = two * (x * z - w * y)
    R[:, 0, 1] = two * (x * y - w * z)
    R[:, 1, 1] = one - two * (x * x - z * z)                            # the reference's sign
    R[:, 2, 1] = two * (y * z + w * x)
    R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    assert same_bits(host["R"], R, nan_equal=True)


def test_fixed_to_float(sets, host):
    inv = np.where(sets["comp"] >= 6, 2.0 ** -28, 2.0 ** -40)
    assert same_bits(host["fixed"], (sets["words"].astype(np.float64) * inv).astype(np.float32), nan_equal=True)
