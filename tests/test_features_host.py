"""The view-space depth of the feature maps (csrc/gs_features.h: gs_view_depth_of, what gs_view_depth runs per gaussian) on the CPU,
against ts[2] of the oracle's preprocess, bit for bit.

The statement is a __host__ __device__ function with contraction off: tests/features_host.cpp is a host build of it, run as a child
process on the means and the view matrix the oracle gets.  Equality is of bit patterns, NaN matching NaN, no tolerance: every operation
is individually rounded on both sides.  Non-finite means are planted: they pass through as IEEE gives them.  Beside it, the host-only
pieces of the feature: the grey export of a depth map."""
import numpy as np
import pytest

from common import bits, host_program, run_host, same_bits, scene_and_cameras
from gaussiansplat_amd import export

N, W, H, DEG, SEED = 4096, 400, 300, 1, 71
NAN, INF = np.float32("nan"), np.float32("inf")


@pytest.fixture(scope="module")
def data(oracle):
    sc, cam, T, P, ocam = scene_and_cameras(N, W, H, DEG, SEED)
    m = sc["means"]
    m[0] = (NAN, 0.0, 0.0); m[1] = (0.0, INF, 0.0); m[2] = (0.0, 0.0, -INF); m[3] = (INF, -INF, 1.0); m[4] = (NAN, INF, -INF)
    m[5] = (3.0e38, 3.0e38, 3.0e38); m[6] = (-0.0, 0.0, -0.0); m[7] = (1.0e-42, -1.0e-42, 1.0e-45)      # beside the overflow, signed zeros, denormals
    m[8] = cam.eye                                                      # t = 0
    pre = oracle.preprocess(sc["means"], sc["scales"], sc["quats"], sc["opacities"], sc["shs"], DEG, ocam)
    return dict(means=np.ascontiguousarray(m, np.float32), T=np.ascontiguousarray(T, np.float32).reshape(-1), ts=pre["ts"])


@pytest.fixture(scope="module")
def host_z(data, tmp_path_factory):
    exe = host_program("features", tmp_path_factory.mktemp("features_host"))
    (z,) = run_host(exe, [], np.uint32(N).tobytes(), [data["T"], data["means"]], [(np.float32, N)])
    return z


def test_the_oracle_depths_are_real_work(data):
    z = data["ts"][:, 2]
    assert data["T"].shape == (16,) and np.count_nonzero(data["T"][[2, 6, 10, 14]]) >= 2
    assert np.isfinite(z[9:]).all() and len(np.unique(z[9:])) > N // 2
    assert np.isnan(z[0]) and not np.isfinite(z[1:5]).any() and np.isfinite(z[5:9]).all() and abs(z[5]) > 1e38


def test_view_depth_statement_equals_the_oracle_bit_for_bit(data, host_z):
    assert same_bits(host_z, data["ts"][:, 2], nan_equal=True)
    fin = np.isfinite(host_z)
    assert np.array_equal(bits(host_z[fin]), bits(data["ts"][fin, 2]))   # finite values: no NaN allowance hides anything


def test_view_depth_statement_is_the_written_order(data, host_z):
    """NumPy float32, one operation at a time, in the header's order: a fused or reordered build would differ in the last bit somewhere."""
    T, m = data["T"], data["means"]
    with np.errstate(all="ignore"):
        s = T[2] * m[:, 0]
        s = s + T[6] * m[:, 1]
        s = s + T[10] * m[:, 2]
        s = s + T[14] * np.float32(1.0)
    assert s.dtype == np.float32 and same_bits(host_z, s, nan_equal=True)


def test_depth_to_gray8():
    d = np.zeros((3, 4), np.float32)
    d[0, 0], d[1, 1], d[2, 3], d[0, 3] = 2.0, 4.0, 6.0, np.nan
    g = export.depth_to_gray8(d, rotate=False)
    assert g.shape == (4, 3, 3) and g.dtype == np.uint8 and np.all(g[..., 0] == g[..., 1]) and np.all(g[..., 0] == g[..., 2])
    assert g[0, 0, 0] == 255 and g[3, 2, 0] == 1 and 1 < g[1, 1, 0] < 255      # near white, far darkest hit, between
    assert g[3, 0, 0] == 0 and g[1, 0, 0] == 0                                  # NaN and empty: black
    assert export.depth_to_gray8(d).shape == (3, 4, 3)                          # rotated as to_rgb8 rotates
    assert not export.depth_to_gray8(np.zeros((2, 2), np.float32)).any()
