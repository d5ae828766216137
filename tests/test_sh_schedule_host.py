"""train.SHDegreeSchedule on the host: the schedule is a pure function of the iteration, and trainStep refuses it for a renderer
without spherical harmonics before anything reaches the GPU."""
import pytest

from gaussiansplat_amd import train as TR


def test_degree_at_boundaries():
    s = TR.SHDegreeSchedule()                                   # the 3DGS recipe: one more band every 1000 iterations, from band 0
    assert [s.degree_at(i) for i in (0, 1, 999, 1000, 1999, 2000, 2999, 3000, 3001, 10 ** 6)] == [0, 0, 0, 1, 1, 2, 2, 3, 3, 3]
    s = TR.SHDegreeSchedule(every=2)
    assert [s.degree_at(i) for i in range(9)] == [0, 0, 1, 1, 2, 2, 3, 3, 3]
    s = TR.SHDegreeSchedule(every=1, start=1)
    assert [s.degree_at(i) for i in range(4)] == [1, 2, 3, 3]
    with pytest.raises(ValueError):
        s.degree_at(-1)


def test_max_degree_clamps():
    s = TR.SHDegreeSchedule(every=10, start=0, max_degree=1)
    assert [s.degree_at(i) for i in (0, 9, 10, 19, 20, 1000)] == [0, 0, 1, 1, 1, 1]
    assert TR.SHDegreeSchedule(every=1, start=2, max_degree=0).degree_at(0) == 0
    assert TR.SHDegreeSchedule(every=5, max_degree=3).degree_at(10 ** 9) == 3


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=-1), dict(every=1.5), dict(start=-1), dict(start=4), dict(max_degree=4), dict(max_degree=-1)])
def test_bad_arguments(kw):
    with pytest.raises(ValueError):
        TR.SHDegreeSchedule(**kw)


def test_train_step_rejects_a_schedule_on_a_2d_renderer():
    from gaussiansplat_amd import renderer as R

    class Untouchable:                                          # any use of the renderer or the loss would raise AttributeError
        pass
    r2d = object.__new__(R.GaussianRenderer2D)                  # a 2-D renderer that never met a GPU
    sched = TR.SHDegreeSchedule(every=2)
    with pytest.raises(ValueError, match="GaussianRenderer3D"):
        TR.trainStep(r2d, None, 0.0, Untouchable(), sh_schedule=sched)
    assert sched.iteration == 0                                 # a refused step is not counted
