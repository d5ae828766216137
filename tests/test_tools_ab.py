"""tools/ab.py: the sweep's order, the variant's environment and the stop rule, over a stub child (tests/ab_stub_child.py).  No GPU."""
import os
import shlex
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT = ["lib_a C1", "lib_a C2", "lib_b C1", "lib_b C2"] * 2


@pytest.fixture
def sweep(tmp_path):
    """run(misbehave, *more) -> (exit status, stdout lines, stderr, the stub's start log): two libraries x C1, C2 x two repetitions"""
    libs = [str(tmp_path / name / "libgsplat_hip.so") for name in ("lib_a", "lib_b")]
    log = tmp_path / "starts.log"
    child = " ".join(shlex.quote(str(w)) for w in (os.path.join(ROOT, "tests", "ab_stub_child.py"), log)) + " {config}"

    def run(misbehave, *more):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "ab.py"), "--libs", *libs, "--configs", "C1,C2", "--reps", "2", "--child", child,
               "--keys", "ms_per_step,stage_ms.composite_bwd", "--log-dir", str(tmp_path / "logs"), *more]
        r = subprocess.run(cmd, env={**os.environ, "AB_STUB_MISBEHAVE": misbehave}, capture_output=True, text=True, timeout=60)
        return r.returncode, r.stdout.splitlines(), r.stderr, log.read_text().splitlines()
    return run


def test_eight_children_in_repetition_major_order_with_the_variants_library(sweep):
    status, out, err, starts = sweep("")
    assert status == 0, err
    assert starts == EIGHT                                                # (the stub logs the folder of its GSPLAT_HIP_LIB)
    assert out == [s + " ms_per_step 1.5000 stage_ms.composite_bwd 1.0000" for s in EIGHT]


def test_third_child_exits_134_and_nothing_is_started_after_it(sweep):
    status, out, err, starts = sweep("3:exit:134")
    assert status != 0 and starts == EIGHT[:3] and len(out) == 2
    assert "exit status 134" in err and "stub start 3" in err            # the reason and the tail of the child's stderr


def test_child_past_its_limit_is_killed_and_ends_the_sweep(sweep):
    status, out, err, starts = sweep("2:sleep:30", "--timeout", "1")
    assert status != 0 and starts == EIGHT[:2] and len(out) == 1
    assert "killed at its limit" in err


def test_child_without_a_json_line_ends_the_sweep(sweep):
    status, out, err, starts = sweep("3:silent")
    assert status != 0 and starts == EIGHT[:3] and len(out) == 2
    assert "no JSON" in err
