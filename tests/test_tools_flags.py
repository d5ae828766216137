"""The measurement tools compile with the build table's flags (tools/_flags.py) and restate none of them.  No GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)


def test_hipcc_flags_is_common_plus_the_sources_entry():
    from _flags import hipcc_flags
    from gaussiansplat_amd import build
    assert len(build.SOURCES) > 30
    for name, extra in build.SOURCES.items():
        assert hipcc_flags(name) == build.COMMON + extra, name


def test_no_tool_restates_a_per_file_flag():
    seen = 0
    for folder, subfolders, files in os.walk(TOOLS):
        subfolders[:] = [d for d in subfolders if d not in ("__pycache__", "abl")]     # (abl: ignored by git, trees of other commits)
        for f in files:
            with open(os.path.join(folder, f), "rb") as fh:
                text = fh.read()
            seen += 1
            for flag in (b"-ffp-contract", b"-fno-slp-vectorize"):
                assert flag not in text, (os.path.join(folder, f), flag)
    assert seen > 50
