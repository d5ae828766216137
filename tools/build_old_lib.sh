#!/bin/bash
# Same-box A/B against an earlier commit's kernels:  tools/build_old_lib.sh COMMIT [TAG=old]  ->  gaussiansplat_amd/lib_TAG/libgsplat_hip.so
# built from that commit's csrc/ + include/, every file with the flags that commit's own gaussiansplat_amd/build.py gives it (SOURCES); ABI functions added since (the ctypes binding
# refuses a library without them) get a stub.  Then: GSPLAT_HIP_LIB=$PWD/gaussiansplat_amd/lib_TAG/libgsplat_hip.so python3 bench.py ...
set -e -o pipefail
C=$1; TAG=${2:-old}
W=$(mktemp -d)
git archive "$C" gaussiansplat_amd/csrc gaussiansplat_amd/build.py include | tar -x -C "$W"
OUT=$PWD/gaussiansplat_amd/lib_$TAG; mkdir -p "$OUT"
grep -q gs_get_bin_path "$W/include/gsplat.h" || echo 'extern "C" int gs_get_bin_path(gs_ctx *c) { return c ? 0 : -1; }' >> "$W/gaussiansplat_amd/csrc/gs_api_debug.hip"
grep -q gs_adam_step "$W/include/gsplat.h" || cat >> "$W/gaussiansplat_amd/csrc/gs_api_debug.hip" <<'STUB'
extern "C" int gs_adam_step(gs_ctx *, const gs_grads *, const gs_grads *, const gs_grads *, const float *, float, float, float, int64_t, int) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_backward_adam(gs_ctx *, const float *, int, const gs_grads *, const gs_grads *, const float *, float, float, float, int64_t, int) { return GS_ERR_UNSUPPORTED; }
STUB
grep -q gs_density_plan "$W/include/gsplat.h" || cat >> "$W/gaussiansplat_amd/csrc/gs_api_debug.hip" <<'STUB'
extern "C" int gs_density_accumulate(gs_ctx *, const void *) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_density_decide(gs_ctx *, const void *, const void *, int32_t *) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_density_plan(gs_ctx *, const int32_t *, int64_t *) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_density_restructure(gs_ctx *, const int32_t *, const float *, const gs_grads *, int32_t, const gs_grads *, const gs_grads *, int64_t) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_opacity_reset(gs_ctx *, float, float *, float *) { return GS_ERR_UNSUPPORTED; }
STUB
grep -q gs_mcmc_plan "$W/include/gsplat.h" || cat >> "$W/gaussiansplat_amd/csrc/gs_api_debug.hip" <<'STUB'
extern "C" int gs_mcmc_plan(gs_ctx *, float, uint64_t *, int32_t *, int64_t *) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_mcmc_sample(gs_ctx *, const uint64_t *, int64_t, const float *, int64_t, int32_t *) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_mcmc_relocate(gs_ctx *, const int32_t *, const int32_t *, int64_t, float, int32_t, const gs_grads *) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_mcmc_noise(gs_ctx *, const float *, float, float, float) { return GS_ERR_UNSUPPORTED; }
extern "C" int gs_mcmc_regularize(gs_ctx *, const gs_grads *, float, float) { return GS_ERR_UNSUPPORTED; }
STUB
objs=()
for s in "$W"/gaussiansplat_amd/csrc/*.hip; do
  b=$(basename "$s" .hip)
  extra=$(python3 -c 'import importlib.util as u, sys; s = u.spec_from_file_location("b", sys.argv[1]); m = u.module_from_spec(s); s.loader.exec_module(m); print(" ".join(m.SOURCES[sys.argv[2]]))' "$W/gaussiansplat_amd/build.py" "$b.hip")
  /opt/rocm/bin/hipcc -O3 -fPIC -std=c++17 --offload-arch=gfx950 -Wno-unused-function $extra -c "$s" -o "$OUT/$b.o" &
  objs+=("$OUT/$b.o")
done
wait
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o "$OUT/libgsplat_hip.so" "${objs[@]}" -ldl
rm -rf "$W"; echo "$OUT/libgsplat_hip.so"
