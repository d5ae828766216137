#!/usr/bin/env python3
"""Same device code?  tools/isa_same.py PARENT.s NEW.s [PARENT_NAME=NEW_NAME ...]

Both files: the gfx950 assembly of one translation unit (hipcc --save-temps, or -S --cuda-device-only) built with build.py's flags, or of several
behind one another when a kernel moved to another unit; a kernel that changed its (mangled) name is compared under the new one.
One line per kernel.  A kernel is `same` when the sequence of its instruction mnemonics and its .amdhsa_next_free_vgpr,
.amdhsa_next_free_sgpr, .amdhsa_private_segment_fixed_size and .amdhsa_group_segment_fixed_size equal the parent's: register names,
block labels and comments may differ.  A kernel whose mnemonics differ is said to have `moved` when the multiset of its mnemonics is the parent's
(instructions changed places, none was added or dropped); it still counts as differing.  The composite kernels' debug-clock instantiations (template argument CLK) may reorder: they
keep their name (which carries the launch bound's waves per SIMD) and their workgroup size, and carry no more scratch than the parent's.
Exit status 1 if a kernel differs or is missing on either side."""
import re, sys

KEYS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """{kernel: {"ops": mnemonics, "wg": max workgroup size, the four KEYS}}"""
    out, body, ops, cur, wg = {}, {}, None, None, None
    for line in open(path):
        s = line.split(";")[0].strip()
        if s.startswith(".amdhsa_kernel "):
            cur = out.setdefault(s.split()[1], {"ops": body.get(s.split()[1], [])})
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and s.startswith(".amdhsa_"):
            cur[s.split()[0][8:]] = s.split()[1]
        elif s.startswith(".max_flat_workgroup_size:"):                # (metadata of a kernel: its .name follows)
            wg = s.split()[1]
        elif s.startswith(".name:") and wg is not None:
            out[s.split()[1]]["wg"], wg = wg, None
        elif re.match(r"[A-Za-z_][\w$.]*:$", s):                       # a function's label: its instructions follow
            body[s[:-1]] = ops = []
        elif s and ops is not None and not s.startswith(".") and not s.endswith(":"):
            ops.append(s.split()[0])
    for name, k in out.items():
        assert k["ops"] and "wg" in k and all(key in k for key in KEYS), "%s: no body, metadata or descriptor found for %s" % (path, name)
    return out


def is_clk(name):                                                   # composite_{fwd,bwd}_kernel<...>: CLK is the 4th / 5th template argument
    m = re.match(r"_Z\d+composite_(fwd|bwd)_kernelI((?:L[bi]\d+E)+)E", name)
    return bool(m) and re.findall(r"L[bi](\d+)E", m.group(2))[3 if m.group(1) == "fwd" else 4] == "1"


rename = dict(a.split("=", 1) for a in sys.argv[3:])                # a kernel that became another: further arguments PARENT_NAME=NEW_NAME
old, new = {rename.get(k, k): v for k, v in kernels(sys.argv[1]).items()}, kernels(sys.argv[2])
bad = 0
for name in sorted(set(old) | set(new)):
    o, n = old.get(name), new.get(name)
    if o is None or n is None:
        ok, verdict = False, "MISSING in " + ("the parent" if o is None else "the new build")
    elif is_clk(name):
        ok = o["wg"] == n["wg"] and int(n[KEYS[2]]) <= int(o[KEYS[2]])
        verdict = ("clk ok" if ok else "CLK DIFFERS") + "  workgroup %s -> %s  scratch %s -> %s  ops %d -> %d" % (o["wg"], n["wg"], o[KEYS[2]], n[KEYS[2]], len(o["ops"]), len(n["ops"]))
    else:
        d = [k for k in KEYS if o[k] != n[k]] + (["mnemonics"] if o["ops"] != n["ops"] else [])
        ok = not d
        moved = d == ["mnemonics"] and sorted(o["ops"]) == sorted(n["ops"])
        verdict = ("same" if ok else "DIFFERS: " + ("moved, multiset equal" if moved else ", ".join(d))) + "  ops %d  vgpr %s sgpr %s scratch %s lds %s" % ((len(n["ops"]),) + tuple(n[k] for k in KEYS))
    bad += not ok
    print("%-100s %s" % (name[:100], verdict))
print("%d kernels, %d differ" % (len(set(old) | set(new)), bad))
sys.exit(1 if bad else 0)
