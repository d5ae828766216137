#!/usr/bin/env python3
"""Same-box A/B of variants on whole bench lines: one sweep of fresh child processes, `for rep: for variant: for config:`, so that clock
ramps and neighbours hit every variant alike.  tools/README.md has the command for every script this replaced.

    tools/ab.py --libs lib lib_x [--configs C3,C5] [--stages fwd=composite_fwd,bwd=composite_bwd] [--isolated]
    tools/ab.py --variant "tile_parts=1: GSPLAT_TILE_PARTS=1" --variant "tile_parts=0: GSPLAT_TILE_PARTS=0" --configs C1,C2
    tools/ab.py --variant "bin_path=3: --bin-path 3" --variant "bin_path=0: --bin-path 0" --keys config.bin_path_of_frame
    tools/ab.py --libs lib lib_x --child tools/loss_prof.py --keys us_per_call

A variant is a label, environment additions and extra child arguments.  --libs names directories under gaussiansplat_amd/ (or paths of
a .so) and sets GSPLAT_HIP_LIB; --variant "LABEL: NAME=VALUE ... --flag ..." gives the words in front of the first flag to the
environment and the rest to the child.  The child is `bench.py --full --config C --steps S --warmup W` without its side lines, unless
--child names another command (a `{config}` in it is filled in); the last line it prints must be JSON.  One line per run: label,
config, ms/frame, the --stages of stage_ms (SHORT=NAME prints NAME as SHORT; default: all that are non-zero), the --keys (dotted paths).

Every child has its own time limit and its stderr is kept in a file under --log-dir.  THE FIRST CHILD THAT EXITS NON-ZERO, IS KILLED AT
ITS LIMIT OR PRINTS NO JSON LINE ENDS THE SWEEP: the tail of its stderr is printed, nothing more is started on the card, the status is 1.
There is no retry.  --isolated then runs tools/abtest.py C3 30 30 (the isolated composite kernels) twice per variant, same rule."""
import argparse
import json
import os
import re
import shlex
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"C1": 60, "C2": 60, "C3": 20, "C4": 8, "C5": 10}              # per config, unless --steps
LIMIT_S = {"C4": 300, "C5": 300}                                       # per child, unless --timeout; every other config 200
SIDE_LINES_OFF = ["--no-cpu-baseline", "--no-literal", "--no-train-iteration", "--no-c4-anchor"]


def lib_variant(name):
    so = os.path.abspath(name) if name.endswith(".so") else os.path.join(ROOT, "gaussiansplat_amd", name, "libgsplat_hip.so")
    return os.path.basename(os.path.dirname(so)), {"GSPLAT_HIP_LIB": so}, []


def word_variant(text):
    label, _, rest = text.partition(":")
    words = shlex.split(rest)
    n_env = next((i for i, w in enumerate(words) if not re.match(r"[A-Za-z_]\w*=", w)), len(words))
    return label.strip(), dict(w.split("=", 1) for w in words[:n_env]), words[n_env:]


def fmt(name, v):
    return "%s %.4f" % (name, v) if isinstance(v, float) else "%s %s" % (name, v)


def run_child(cmd, env, limit, err_path, want_json=True):
    """-> the child's stdout (want_json: its last line, parsed), or None when it exited non-zero, was killed at its limit or printed
    no JSON line: then the reason and the tail of its stderr are printed"""
    with open(err_path, "w") as err:
        p = subprocess.Popen(cmd, cwd=ROOT, env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=err, text=True, start_new_session=True)
        try:
            out, why = p.communicate(timeout=limit)[0], p.returncode and "exit status %d" % p.returncode
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGTERM)                           # the child and whatever it started; ten seconds to go, as `timeout -k 10`
            try:
                p.communicate(timeout=10)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.communicate()
            why = "killed at its limit of %g s" % limit
    if not why and want_json:
        try:
            return json.loads(out.strip().splitlines()[-1])
        except (IndexError, ValueError):
            why = "its last line is no JSON"
    if not why:
        return out
    print("ab.py: %s: %s; stderr (%s) ends:" % (" ".join(cmd), why, err_path), file=sys.stderr)
    with open(err_path) as fh:
        sys.stderr.write("".join(fh.readlines()[-20:]))
    print("ab.py: the sweep ends here", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--libs", nargs="+", default=[])
    ap.add_argument("--variant", action="append", default=[], metavar='"LABEL: NAME=VALUE ... --flag ..."')
    ap.add_argument("--configs", default=None, help="comma-separated (bench child: default C3)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=None, help="default per config: C1 C2 60, C3 20, C4 8, C5 10")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=None, help="seconds per child (default 200; 300 for C4 and C5)")
    ap.add_argument("--stages", default="", help="stage_ms keys to print, NAME or SHORT=NAME (default: all non-zero)")
    ap.add_argument("--keys", default="", help="further keys of the JSON line to print, dotted paths")
    ap.add_argument("--bench-args", default="", help='further bench.py arguments of every variant, as --bench-args="--bin-path 2"')
    ap.add_argument("--child", default="", help="a command in place of bench.py (run with this interpreter when it names a .py)")
    ap.add_argument("--isolated", action="store_true", help="then tools/abtest.py C3 30 30, twice per variant")
    ap.add_argument("--log-dir", default=os.path.join(ROOT, "out", "ab"))
    a = ap.parse_args()
    variants = [lib_variant(n) for n in a.libs] + [word_variant(t) for t in a.variant] or [("default", {}, [])]
    configs = a.configs.split(",") if a.configs else ([None] if a.child else ["C3"])
    stages = [s.partition("=")[::2] if "=" in s else (s, s) for s in a.stages.split(",") if s]
    os.makedirs(a.log_dir, exist_ok=True)
    logs = ("%s/%03d.stderr" % (a.log_dir, i) for i in range(1, 10 ** 6))
    for rep in range(a.reps):
        for label, env, words in variants:
            for c in configs:
                if a.child:
                    cmd = shlex.split(a.child.replace("{config}", c or "")) + words
                    cmd = [sys.executable] + cmd if cmd[0].endswith(".py") else cmd
                else:
                    cmd = [sys.executable, "bench.py", "--full", "--config", c, "--steps", str(a.steps or STEPS.get(c, 20)), "--warmup", str(a.warmup),
                           *SIDE_LINES_OFF, *shlex.split(a.bench_args), *words]
                d = run_child(cmd, env, a.timeout or LIMIT_S.get(c, 200), next(logs))
                if d is None:
                    return 1
                cols = [label] + ([c] if c else [])
                if not a.child:
                    s = d["stage_ms"]
                    cols.append("ms/frame %.4f" % d["ms_per_step"])
                    cols += [fmt(short, s[k]) for short, k in stages] if stages else [fmt(k, v) for k, v in s.items() if v]
                for path in filter(None, a.keys.split(",")):
                    v = d
                    for k in path.split("."):
                        v = v[k]
                    cols.append(fmt(path, v))
                print(" ".join(cols), flush=True)
    for rep in range(2 if a.isolated else 0):
        for label, env, _ in variants:
            print("== isolated kernels " + label, flush=True)
            out = run_child([sys.executable, "tools/abtest.py", "C3", "30", "30"], {**env, "AB_TMIN": "1e-5", "AB_ROUNDS": "4"}, a.timeout or 120, next(logs),
                            want_json=False)
            if out is None:
                return 1
            print(out, end="", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
