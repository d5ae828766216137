"""renderer.grads_layout is the layout initGrads / initGrads2D build: the offsets it returns are the element offsets of the views, the total is
the buffer's length, and the views tile the buffer without overlap.  CPU tensors; no device."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _check(R, grads, widths, n):
    offsets, total = R.grads_layout(widths, n)
    views = R.grads_views(grads)
    assert len(offsets) == len(views) == 5 and total == grads.flat.numel() == sum(widths) * n
    assert R.layout_of(grads) == (offsets, total)
    covered = np.zeros(total, np.int64)
    for o, w, v in zip(offsets, widths, views):
        assert tuple(v.shape) == (n, w) and v.is_contiguous()
        assert v.storage_offset() - grads.flat.storage_offset() == o            # element offsets, straight from torch
        covered[o:o + n * w] += 1
    assert (covered == 1).all()                                                # no overlap, nothing left over
    if total:                                                                  # and the views ARE the buffer: a mark through one shows in the other
        for k, v in enumerate(views):
            v.fill_(float(k + 1))
        want = np.concatenate([np.full(n * w, k + 1, np.float32) for k, w in enumerate(widths)])
        assert np.array_equal(grads.flat.numpy(), want)
    s = R.grads_struct(grads.flat, offsets)
    got = (s.d_means, s.d_scales, s.d_quats, s.d_opacities, s.d_shs)
    if total:
        assert [int(p or 0) for p in got] == [v.data_ptr() if v.numel() else grads.flat.data_ptr() + 4 * o for v, o in zip(views, offsets)]


@pytest.mark.parametrize("n,k3", list(itertools.product((0, 1, 5), (3, 12, 48))))
def test_grads_layout_is_the_layout_of_initGrads(n, k3):
    from gaussiansplat_amd import renderer as R
    d = R.SplatData3D(means=torch.zeros(n, 3), scales=torch.zeros(n, 3), shs=torch.zeros(n, k3), quaternions=torch.zeros(n, 4), opacities=torch.zeros(n, 1))
    _check(R, R.initGrads(d), (3, 3, 4, 1, k3), n)


@pytest.mark.parametrize("n", (0, 1, 5))
def test_grads_layout_is_the_layout_of_initGrads2D(n):
    from gaussiansplat_amd import renderer as R
    d = R.SplatData2D(means=torch.zeros(n, 2), scales=torch.zeros(n, 2), rotations=torch.zeros(n, 1), opacities=torch.zeros(n, 1), colors=torch.zeros(n, 3))
    _check(R, R.initGrads2D(d), (2, 2, 1, 1, 3), n)


def test_grads_layout_is_pure_arithmetic():
    from gaussiansplat_amd import renderer as R
    assert R.grads_layout((3, 3, 4, 1, 48), 7) == ((0, 21, 42, 70, 77), 413)
    assert R.grads_layout((2, 2, 1, 1, 3), 0) == ((0, 0, 0, 0, 0), 0)
