"""Build libgsplat_hip.so in-tree with hipcc for gfx950 (no CMake, no JIT cache).

    python -m gaussiansplat_amd.build [--force] [--tag NAME -DMACRO=... ...]

--tag NAME builds lib_NAME/libgsplat_hip.so with the given -D macros (e.g. --tag seg1k -DL2_SEG=1024): a variant for a same-box
A/B run, loaded with GSPLAT_HIP_LIB=.../lib_NAME/libgsplat_hip.so (tools/ab.py --libs lib lib_NAME).  The kernel variants that lost their A/B
in rounds 1-3 (persistent ticket queues, the reduction tree, the software-pipelined backward, the 64-VGPR forward) and their
environment switches are no longer in the tree: profiles/HISTORY.md names the commit that last had them.

The preprocess translation units are compiled with -ffp-contract=off (numeric spec: tile ids
and depth keys must be bit-identical to the CPU oracle).  The composite kernels turn contraction
off themselves (`#pragma clang fp contract(off)` at the top of gs_composite.hip: only the fmaf()
calls written there fuse, so that every instantiation rounds a pixel's T the same way) and are
built without the SLP vectoriser; their pixels and gradients are tolerance-checked.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(OUT_DIR, "libgsplat_hip.so")
ARCH = "gfx950"

SOURCES = {
    "gs_preprocess.hip": ["-ffp-contract=off"],
    "gs_preprocess2d.hip": ["-ffp-contract=off"],
    "gs_preprocess_bwd.hip": [],
    # same flags as gs_preprocess_bwd.hip: the two kernels that rebuild SH gradients from views share one body (gs_sh_views_body.inc, with the
    # basis text gs_sh_basis.inc inside it) and must round alike -- the text is contracted as the including translation unit is built
    "gs_touched.hip": [],
    # the one scan of the chunk words (touched rows, density plan, MCMC plan): integers only
    "gs_chunk.hip": [],
    "gs_sort.hip": [],
    "gs_bin2.hip": [],
    "gs_bin3.hip": [],
    "gs_bin_small.hip": [],
    # no SLP vectoriser: a v_pk_*_f32 issues at the cost of two plain operations on gfx950, and forming the pairs costs moves
    # (C3 1.328 -> 1.294 ms, C5 4.38 -> 4.26, same box, profiles/r04q_ab_no_slp.log; round 2's kernels had measured the opposite)
    "gs_composite.hip": ["-fno-slp-vectorize"],
    # the launch orders, the summing kernels and the clock probe: once part of gs_composite.hip, built as that unit is so that their code stays what it was
    "gs_order.hip": ["-fno-slp-vectorize"],
    # the SLP vectoriser turns the stencil into v_pk_* (no faster than two plain ops on gfx950) plus 270 register moves per loop body
    "gs_loss.hip": ["-fno-slp-vectorize"],
    # Adam: the per-float update must round exactly as documented in include/gsplat.h (and as gs_sh_bwd_kernel's fused form does)
    "gs_adam.hip": ["-ffp-contract=off"],
    # density control: statistics, decisions and the children of a split are specified operation by operation (tests/density_ref.py matches bit for bit)
    "gs_density.hip": ["-ffp-contract=off"],
    "gs_api_density.hip": ["-ffp-contract=off"],
    # background colour: blend and target compositor are specified as single fp32 operations (NumPy float32 matches bit for bit)
    "gs_background.hip": ["-ffp-contract=off"],
    # point-cloud initialisation: d2, the box bound and the mean are specified operation by operation (tests/knn_ref.py matches bit for bit)
    "gs_knn.hip": ["-ffp-contract=off"],
    "gs_api_knn.hip": ["-ffp-contract=off"],
    # feature maps: the view-space depth is the preprocess's own statement (GS_ARR_TS row 2, bit for bit), its adjoint one multiply and one add
    "gs_features.hip": ["-ffp-contract=off"],
    "gs_api_features.hip": [],
    # camera gradient: the statement (gs_camera_grad.h) and the two reduction kernels round operation by operation, as tests/camera_grad_host.cpp does on the CPU
    "gs_camera.hip": ["-ffp-contract=off"],
    "gs_api_camera.hip": [],
    # evaluation metrics: double arithmetic throughout, held to 1e-10 against a float64 restatement, not bit for bit: contraction stays on
    "gs_metrics.hip": [],
    "gs_api_metrics.hip": [],
    # per-view exposure: the affine, its adjoints and the row's Adam step are specified operation by operation (tests/exposure_ref.py matches bit for bit)
    "gs_exposure.hip": ["-ffp-contract=off"],
    "gs_api_exposure.hip": [],
    # per-view bilateral grid: cell, slice, affine and adjoints are specified operation by operation (tests/bilagrid_ref.py matches bit for bit)
    "gs_bilagrid.hip": ["-ffp-contract=off"],
    "gs_api_bilagrid.hip": [],
    # MCMC densification: weights, draws, noise and regularisers are specified operation by operation (tests/mcmc_ref.py matches bit for bit)
    "gs_mcmc.hip": ["-ffp-contract=off"],
    "gs_api_mcmc.hip": ["-ffp-contract=off"],
    "gs_api.hip": [],
    "gs_api_bin.hip": [],
    "gs_api_composite.hip": [],
    "gs_api_comm.hip": [],
    "gs_api_touched.hip": [],
    "gs_api_debug.hip": [],
}
COMMON = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _deps() -> float:
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    hdrs.append(os.path.join(HERE, "..", "include", "gsplat.h"))
    return max(os.path.getmtime(h) for h in hdrs)


def build(force: bool = False, verbose: bool = False, tag: str = "", defines=()) -> str:
    """tag / defines: a variant build for same-box A/B runs (e.g. tag="p48", defines=["-DGS_PAYLOAD_QUADS=3"] -> lib_p48/)."""
    out_dir = os.path.join(HERE, "lib_" + tag) if tag else OUT_DIR
    lib = os.path.join(out_dir, "libgsplat_hip.so")
    os.makedirs(out_dir, exist_ok=True)
    hipcc = _hipcc()
    hdr_time = _deps()
    objs, jobs = [], []
    for src, extra in SOURCES.items():
        extra = [*extra, *defines]
        s = os.path.join(CSRC, src)
        o = os.path.join(out_dir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), hdr_time):
            jobs.append([hipcc, *COMMON, *extra, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if jobs or force or not os.path.exists(lib):
        run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib, *objs, "-ldl"])
    return lib


if __name__ == "__main__":
    tag = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else ""
    print(build(force="--force" in sys.argv, verbose=True, tag=tag,
                defines=[a for a in sys.argv[1:] if a.startswith("-D") or a.startswith("-f") or a.startswith("-mllvm") or a.startswith("-amdgpu")]))
