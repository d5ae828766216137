"""hipcc flags of one translation unit, read from the build table (gaussiansplat_amd/build.py: COMMON + SOURCES[name]).

    from _flags import hipcc_flags;  hipcc_flags("gs_composite.hip")
    python3 tools/_flags.py gs_composite.hip        (one line, for shell scripts)

Imports gaussiansplat_amd.build only: neither torch nor a GPU is needed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from gaussiansplat_amd import build as _build  # noqa: E402


def hipcc_flags(name):
    return _build.COMMON + _build.SOURCES[name]


if __name__ == "__main__":
    print(" ".join(hipcc_flags(sys.argv[1])))
