#!/bin/bash
# GPU box: the whole -m gpu suite, then same-box A/B of the default build against `--list-cap 1` at C3 and C5 (round 4).
# usage (from the repo root): [OUT=folder] bash tools/gpu_check.sh [tag]
tag=${1:-chk}
O=${OUT:-out}                        # output folder
mkdir -p "$O"
python -m pytest tests -q -m gpu --durations=8 > $O/${tag}_tests.log 2>&1; echo rc=$? >> $O/${tag}_tests.log
tail -15 $O/${tag}_tests.log
for rep in 1 2; do
for c in "" "--list-cap 1"; do
  k=$(echo "$c" | tr -d " -")
  python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-literal --no-train-iteration --no-c4-anchor $c > $O/${tag}_c3${k}_$rep.json 2>$O/${tag}_b.err
  python bench.py --full --config C5 --steps 10 --warmup 3 --no-cpu-baseline --no-literal $c > $O/${tag}_c5${k}_$rep.json 2>>$O/${tag}_b.err
done
done
python - "$tag" "$O" <<'PY'
import glob, json, sys
for f in sorted(glob.glob("%s/%s_c*.json" % (sys.argv[2], sys.argv[1]))):
    try:
        d = json.loads(open(f).read().strip().splitlines()[-1])
        c = d["config"]
        print(f, "ms", round(d["ms_per_step"], 4), "capped", c["lists_capped"], "listed", c["listed_entries"], "of", c["instances"], "ext", c["list_segments_appended_by_waves"],
              {k: v for k, v in d["stage_ms"].items() if v > 0})
    except Exception as e:
        print(f, "ERR", e)
PY
