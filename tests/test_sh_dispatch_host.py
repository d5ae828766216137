"""gs_sh_dispatch (csrc/gs_sh.h): the one place that turns (active SH degree, row stride) into an instantiation of an SH kernel.

Host code, compiled alone and run without a device: every launcher of an SH kernel goes through it, so what it refuses and which
(degree, strided) pair it hands on is pinned here against the rule written out independently: degree 0..3, stride >= 3 K, a stride above
3 K (an active degree below the stored one) only for degrees 0..2 -- there is no strided degree-3 kernel."""
import subprocess

from common import host_program


def test_dispatch_validates_once_and_names_existing_instantiations_only(tmp_path_factory):
    exe = host_program("sh_dispatch", tmp_path_factory.mktemp("sh_dispatch_host"))
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [line.split() for line in out if line]
    assert len(rows) == 8 * 82
    seen = set()
    for deg, stride, verdict, d, s in rows:
        deg, stride, d, s = int(deg), int(stride), int(d), int(s)
        k3 = 3 * (deg + 1) ** 2
        valid = 0 <= deg <= 3 and (stride == k3 or (stride > k3 and deg <= 2))
        if valid:
            assert (verdict, d, s) == ("called", deg, int(stride > k3)), (deg, stride, verdict, d, s)
            seen.add((d, s))
        else:
            assert (verdict, d, s) == ("invalid", -1, -1), (deg, stride, verdict, d, s)
    assert seen == {(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1)}
