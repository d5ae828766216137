#!/bin/bash
# Same-box A/B against an earlier commit's kernels:  tools/build_old_lib.sh COMMIT [TAG=old]  ->  gaussiansplat_amd/lib_TAG/libgsplat_hip.so
# built from that commit's csrc/ + include/, every file with the flags that commit's own gaussiansplat_amd/build.py gives it (SOURCES); ABI functions added since (the ctypes binding
# refuses a library without them) get a generated stub.  Then: tools/ab.py --libs lib_TAG lib, or GSPLAT_HIP_LIB=$PWD/gaussiansplat_amd/lib_TAG/libgsplat_hip.so python3 bench.py ...
# The one way to build another commit's library: it supersedes build_ref_lib.sh, whose hand-kept copy of the per-file flags had gone stale.
set -e -o pipefail
C=$1; TAG=${2:-old}
W=$(mktemp -d)
git archive "$C" gaussiansplat_amd/csrc gaussiansplat_amd/build.py include | tar -x -C "$W"
OUT=$PWD/gaussiansplat_amd/lib_$TAG; mkdir -p "$OUT"
# a stub for every function today's header declares and that commit's does not, written from today's prototypes (tests/abi_header.py: the
# header reader of the ABI tests).  Pointers become const void *, which C linkage makes harmless and which needs no type the old header lacks.
python3 - "$(dirname "$0")/../tests" "$W/include/gsplat.h" >> "$W/gaussiansplat_amd/csrc/gs_api_debug.hip" <<'PY'
import sys
sys.path.insert(0, sys.argv[1])
from abi_header import _c_kind, _c_prototypes
ctype = {"i32": "int32_t", "i64": "int64_t", "f32": "float", "f64": "double", "ptr": "const void *"}
old = _c_prototypes(sys.argv[2])
for name, (ret, args) in _c_prototypes().items():
    if name not in old:
        assert ret == "int", name
        body = "return a0 ? 0 : -1;" if name == "gs_get_bin_path" else "return GS_ERR_UNSUPPORTED;"      # (a ctx of that commit took path 0)
        params = ", ".join("%s a%d" % (ctype[_c_kind(a)[0]], i) for i, a in enumerate(args))
        print('extern "C" int %s(%s) { %s }' % (name, params, body))
PY
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
