"""Point-cloud initialisation without a GPU: the 3-NN pipeline of csrc/gs_knn.hip on the CPU, and the host side of the feature.

tests/knn_host.cpp is a host build of the statements in csrc/gs_knn.h (contraction off) that runs the WHOLE pipeline serially -- keys, a
stable sort, boxes, the bound-pruned search -- on every cloud of tests/knn_ref.py.  Its results must equal the NumPy brute force bit for
bit, NaN matching NaN: both sides round every operation on its own, and the search may skip a box only where no value in it could change
the three smallest.  It also reports how many (query, box) pairs it pruned and opened: on the uniform cloud both must be non-zero, so that
neither "opened everything" nor "pruned everything" passes.  Then ply.load_points, PointCloud's refusals and camera.scene_extent."""
import os
import re

import numpy as np
import pytest

import knn_ref as K
from common import bits, host_program, run_host, same_bits
from gaussiansplat_amd import backend
from gaussiansplat_amd import build as gbuild
from gaussiansplat_amd import ply
from gaussiansplat_amd.camera import default_camera, scene_extent
from gaussiansplat_amd.pointcloud import PointCloud


@pytest.fixture(scope="module")
def clouds():
    return K.clouds()


@pytest.fixture(scope="module")
def refs(clouds):
    return {name: K.knn_mean_dist2(p) for name, p in clouds.items()}


@pytest.fixture(scope="module")
def host(clouds, tmp_path_factory):
    exe = host_program("knn", tmp_path_factory.mktemp("knn_host"))
    names = list(clouds)
    arrays = [a for name in names for a in (np.uint32(len(clouds[name])), np.asarray(clouds[name], np.float32))]
    (flat,), printed = run_host(exe, [], np.uint32(len(names)).tobytes(), arrays, [(np.float32, sum(len(clouds[name]) for name in names))], stdout=True)
    out, p = {}, 0
    lines = printed.strip().splitlines()
    assert len(lines) == len(names)
    for k, name in enumerate(names):
        n = len(clouds[name])
        m = re.fullmatch(r"cloud (\d+) n (\d+) pruned (\d+) opened (\d+)", lines[k])
        assert m and int(m.group(1)) == k and int(m.group(2)) == n, lines[k]
        out[name] = dict(dist2=flat[p:p + n], pruned=int(m.group(3)), opened=int(m.group(4)))
        p += n
    assert p == len(flat)
    return out


def test_box_constant_agrees():
    hdr = open(os.path.join(gbuild.CSRC, "gs_knn.h")).read()
    assert int(re.search(r"#define GS_KNN_BOX\s+(\d+)", hdr).group(1)) == backend.KNN_BOX == K.BOX


def test_every_cloud_fits_the_cpu_pipeline_and_the_reference_shows_its_case(clouds, refs):
    assert {"uniform4", "uniform5", "uniform63", "uniform64", "uniform65", "uniform4097", "clustered", "duplicates", "all_identical", "line",
            "plane", "lattice", "nonfinite", "too_few", "overflow"} <= set(clouds)
    for name, p in clouds.items():
        assert p.dtype == np.float32 and p.shape[1] == 3 and len(p) <= 4097
        K.check_planted(name, p, refs[name])


def test_cpu_pipeline_matches_brute_force_bit_for_bit(clouds, refs, host):
    for name in clouds:
        got, want = host[name]["dist2"], refs[name]
        bad = np.flatnonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


def test_the_search_prunes_and_opens(host, clouds):
    h = host["uniform4097"]
    print("uniform4097: (query, box) pairs pruned", h["pruned"], "opened", h["opened"])
    assert h["pruned"] > 0 and h["opened"] > 0
    nb = (4097 + K.BOX - 1) // K.BOX
    assert h["pruned"] + h["opened"] == 4097 * (nb - 1)                  # every query decides on every box but its own
    # all points identical: the own box fills the triple with zeros and bound >= b2 prunes everything else (with > it would be quadratic)
    assert host["all_identical"]["opened"] == 0 and host["all_identical"]["pruned"] > 0


# ---------------------------------------------------------------- ply.load_points
def write_points_ply(path, pts, rgb=None, extra=True):
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if extra:
        cols += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb is not None:
        cols += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    tab = np.zeros(len(pts), dtype=cols)
    for i, k in enumerate("xyz"):
        tab[k] = pts[:, i]
    if rgb is not None:
        for i, k in enumerate(("red", "green", "blue")):
            tab[k] = rgb[:, i]
    tname = {"<f4": "float", "u1": "uchar"}
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(pts)).encode())
        fh.write("".join(f"property {tname[t]} {k}\n" for k, t in cols).encode())
        fh.write(b"end_header\n")
        tab.tofile(fh)


def test_load_points_with_and_without_colours(tmp_path):
    rng = np.random.default_rng(11)
    pts = rng.standard_normal((37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    rgb[0], rgb[1] = 0, 255
    write_points_ply(str(tmp_path / "c.ply"), pts, rgb)
    pc = ply.load_points(str(tmp_path / "c.ply"))
    assert isinstance(pc, PointCloud) and len(pc) == 37 and pc.sh_degree == 3 and pc.opacity == 0.1
    assert same_bits(pc.points, pts, nan_equal=True)
    assert pc.colors.dtype == np.float32 and same_bits(pc.colors, rgb.astype(np.float32) / np.float32(255.0), nan_equal=True)
    assert pc.colors[0].tolist() == [0.0, 0.0, 0.0] and pc.colors[1].tolist() == [1.0, 1.0, 1.0]
    write_points_ply(str(tmp_path / "p.ply"), pts, None, extra=False)
    pc = ply.load_points(str(tmp_path / "p.ply"), sh_degree=1, opacity=0.25)
    assert pc.colors is None and same_bits(pc.points, pts, nan_equal=True) and pc.sh_degree == 1 and pc.opacity == 0.25


def test_pointcloud_refusals():
    pts = K.uniform(10, 1)
    col = K.uniform(10, 2)
    PointCloud(pts, col)
    PointCloud(pts[:4], None, sh_degree=0, opacity=0.5)
    for bad in (np.float32("nan"), np.float32("inf"), -np.float32("inf")):
        p = pts.copy()
        p[3, 1] = bad
        with pytest.raises(ValueError):
            PointCloud(p, col)
    with pytest.raises(ValueError):
        PointCloud(pts[:3], col[:3])                                     # n < 4
    with pytest.raises(ValueError):
        PointCloud(pts.reshape(-1), None)
    for v in (-1e-3, 1.001, np.float32("nan")):
        c = col.copy()
        c[0, 2] = v
        with pytest.raises(ValueError):
            PointCloud(pts, c)
    with pytest.raises(ValueError):
        PointCloud(pts, col[:5])
    for deg in (-1, 4, 1.5, True):
        with pytest.raises(ValueError):
            PointCloud(pts, col, sh_degree=deg)
    for op in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            PointCloud(pts, col, opacity=op)


def test_scene_extent_by_hand():
    cams = []
    for eye in ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, 0.0, 4.0)):
        c = default_camera()
        c.eye = np.array(eye, np.float32)
        cams.append(c)
    # mean (1, 1, 1); the origin is sqrt(3) away, the other three sqrt(9 + 1 + 1) = sqrt(11)
    assert scene_extent(cams) == 1.1 * np.sqrt(np.float64(11.0))
    assert scene_extent(cams[:1]) == 0.0
    from gaussiansplat_amd.density import density_params
    density_params(scene_extent=scene_extent(cams))
