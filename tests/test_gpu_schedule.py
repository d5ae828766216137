"""gs_config.schedule only changes which wave processes which tile and when: every mode must give the same image and
transmittance bit for bit, the same deterministic-mode gradients bit for bit (so no tile is skipped or processed twice),
and float-atomic gradients equal to atomic-order noise."""
import numpy as np
import pytest

from common import GRADS, hip_context, rel_l2, scene_and_cameras

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,W,H,deg,scale_shift,t_min", [
    (20_000, 400, 304, 2, 0.6, 1e-5),          # 25 x 19 tiles (gx % 8 != 0), pixels freeze
    (9_000, 256, 144, 1, 0.0, 0.0),            # literal: every list walked to the end
    (30_000, 648, 200, 3, 0.9, 1e-3),          # 41 x 13 tiles, ragged right edge
])
def test_all_schedules_agree(n, W, H, deg, scale_shift, t_min):
    from gaussiansplat_amd import synthetic
    sc, cam, T, P, ocam = scene_and_cameras(n, W, H, deg, 31)
    sc["scales"] = sc["scales"] + np.float32(scale_shift)
    dC = synthetic.make_dC(W, H, 31)
    ref = {}
    for det in (True, False):
        for schedule, slot in ((1, -1), (3, -1), (3, 5), (4, -1), (0, 7)):
            ctx = hip_context(sc, cam, T, P, W, H, deg, t_min=t_min, deterministic=det, schedule=schedule, slab_mode=0,
                              debug_flags=2)                        # GS_DEBUG_ALWAYS_ORDER: these grids are smaller than the wave slots
            ctx.set_view_slot(slot)
            out = None
            for frame in range(1 if schedule == 1 else 3):               # later frames launch the forward by what the slot / the previous frame measured
                ctx.preprocess(); ctx.bin()
                img, tr = ctx.forward_host()
                g = ctx.grads_alloc(); ctx.backward(dC, g)
                out = (img, tr, ctx.grads_read(g, deg), ctx.work_counters_ex())
            ctx.close()
            if det not in ref:
                ref[det] = out
                continue
            r = ref[det]
            assert np.array_equal(out[0], r[0]) and np.array_equal(out[1], r[1]), schedule
            assert out[3] == r[3], schedule
            for k in GRADS:
                if det:
                    assert np.array_equal(out[2][k], r[2][k]), (schedule, k)
                else:
                    assert rel_l2(out[2][k].reshape(-1), r[2][k].reshape(-1)) <= 1e-5, (schedule, k)
