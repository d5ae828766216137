"""The composite-forward stage at a BASELINE config (default C3) over black, with the tree in the CURRENT DIRECTORY -- so that the same
loop can be run from a checkout of another commit for a same-box A/B (alternate the two, a fresh process per run):

    cd CHECKOUT && python /path/to/tools/fwd_stage_time.py NAME [CONFIG]

One JSON line: median / min / max of gs_get_stage_times over 30 frames after 4 untimed ones.  Uses nothing newer than profile_stages.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())


def main():
    import torch
    from gaussiansplat_amd import renderer as R, synthetic
    name = sys.argv[1] if len(sys.argv) > 1 else "tree"
    config = sys.argv[2] if len(sys.argv) > 2 else "C3"
    n, W, H, deg = synthetic.CONFIGS[config]
    scene = synthetic.make_scene(n, W, H, deg, seed=1234 + list(synthetic.CONFIGS).index(config))
    cam = synthetic.scene_camera(W)
    r = R.getRenderer("GAUSSIAN_3D", (W, H, 3), (16, 16), None, scene, profile_stages=True)
    ts = []
    for i in range(4 + 30):
        tps = R.preprocess(r, cam); R.compactIdxs(r); R.forward(r, tps)
        torch.cuda.synchronize()
        if i >= 4:
            ts.append(r.ctx.stage_times()["composite_fwd"])
    print(json.dumps(dict(tree=name, config=config, frames=len(ts), unit="ms", median=statistics.median(ts), min=min(ts), max=max(ts))))


if __name__ == "__main__":
    main()
