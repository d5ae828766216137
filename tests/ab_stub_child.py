"""Stands for bench.py under tools/ab.py (tests/test_tools_ab.py): `ab_stub_child.py LOG CONFIG` appends "<directory of GSPLAT_HIP_LIB>
CONFIG" to LOG and prints one JSON line.  AB_STUB_MISBEHAVE="N:exit:134", "N:silent" or "N:sleep:30" makes the N-th start (counted in
LOG) exit with that status, print nothing, or sleep that many seconds first."""
import json
import os
import sys
import time

log, config = sys.argv[1:3]
label = os.path.basename(os.path.dirname(os.environ.get("GSPLAT_HIP_LIB", "")))
with open(log, "a") as fh:
    fh.write("%s %s\n" % (label, config))
with open(log) as fh:
    nth = len(fh.readlines())
n, _, what = (os.environ.get("AB_STUB_MISBEHAVE") or "0:").partition(":")
what = what if int(n) == nth else ""
print("stub start %d" % nth, file=sys.stderr)
if what.startswith("exit"):
    sys.exit(int(what.split(":")[1]))
if what.startswith("sleep"):
    time.sleep(float(what.split(":")[1]))
if what != "silent":
    print("a line in front of the result")
    print(json.dumps({"ms_per_step": 1.5, "stage_ms": {"composite_fwd": 0.5, "composite_bwd": 1.0, "idle": 0.0}}))
