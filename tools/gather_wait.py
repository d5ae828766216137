#!/usr/bin/env python3
"""Does the next batch's row gather stay in flight over the per-entry loops?   tools/gather_wait.py [--rev REV] [--same-as REV]

Compiles gaussiansplat_amd/csrc/gs_composite.hip (of the working tree, or of git revision REV with that revision's headers) for gfx950
with build.py's flags, to assembly, and prints one line per composite instantiation and gather site.  A gather site is a basic block with
the four global_load_dwordx4 of one payload row (offsets 0, 16, 32, 48 from one address); its sixteen destination registers are the
gathered registers.  From the site the tool follows the control flow forward -- the rest of the site's block, then every block reachable
from it -- without entering a gather site or the block that guards one (the one that ends in the s_cbranch_execz round the site: the
staging code runs into it), and keeps the blocks from which a per-entry block (one that reads the staged entries, ds_read_b128) can still
be reached under the same rule.  In that region it counts

  waits   s_waitcnt with a vmcnt term,
  moves   v_mov_* that name a gathered register,
  other   other instructions that name a gathered register,

so 0 / 0 / 0 says: nothing waits for the gather and nothing touches its registers until the last per-entry loop is left.  The site before
the walk's first batch feeds the staging directly; it has no such region and prints `region 0 blocks`.  Registers, scratch and occupancy
are the compiler's kernel-resource-usage remarks, read as tools/kernel_regs.sh reads them.  --same-as REV also compiles REV and runs
tools/isa_same.py (parent = REV) on the two assemblies, which says which instantiations kept their code.
The tool reads waits and register names only; it looks for no particular instruction beyond the loads, moves and waits named above."""
import argparse, os, re, subprocess, sys, tempfile

from _flags import ROOT, hipcc_flags

FLAGS = hipcc_flags("gs_composite.hip")
REMARK = re.compile(r"remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\d+)")


def compile_asm(rev, out):
    """-> (path of the .s, {mangled kernel: remarks})"""
    if rev:
        src_root = tempfile.mkdtemp(prefix="gather_wait_")
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "gaussiansplat_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", src_root], input=tar, check=True)
    else:
        src_root = ROOT
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, *FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(src_root, "gaussiansplat_amd/csrc/gs_composite.hip"), "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    regs, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = regs.setdefault(m.group(1), {})
        m = REMARK.search(line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out, regs


def kernel_bodies(path):
    """{mangled composite kernel: its instruction lines and labels}"""
    out, cur = {}, None
    for line in open(path):
        s = line.split(";")[0].rstrip()
        m = re.match(r"(_Z\d+composite_(?:fwd|bwd)_kernel\w+):$", s)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            if s.startswith(".Lfunc_end"):
                cur = None
            elif s.strip() and not s.strip().startswith("."):
                cur.append(s.strip())
            elif re.match(r"\.LBB\d+_\d+:$", s):
                cur.append(s)
            elif re.match(r"\s*; %bb\.\d+:", line):                     # a block entered by falling through only
                cur.append("%" + line.split("%")[1].split(":")[0] + ":")
    return out


def blocks_of(lines):
    """basic blocks: [{"name", "ins": [...], "succ": [indices]}]"""
    blocks, alias = [{"name": "entry", "ins": []}], {}
    for s in lines:
        if s.endswith(":"):
            if blocks[-1]["ins"]:
                blocks.append({"name": s[:-1], "ins": []})
            else:                                                       # (the empty block opened behind a branch, or the kernel's first)
                alias[blocks[-1]["name"]] = s[:-1]                      # (two labels on one block)
                blocks[-1]["name"] = s[:-1]
            continue
        blocks[-1]["ins"].append(s)
        if s.split()[0] in ("s_branch", "s_endpgm") or s.startswith("s_cbranch"):
            blocks.append({"name": "after_%d" % len(blocks), "ins": []})
    index = {b["name"]: i for i, b in enumerate(blocks)}
    for old in alias:
        new = old
        while new in alias:
            new = alias[new]
        index[old] = index[new]
    for i, b in enumerate(blocks):
        last = b["ins"][-1] if b["ins"] else ""
        op = last.split()[0] if last else ""
        nxt = [i + 1] if i + 1 < len(blocks) else []
        if op == "s_branch":
            b["succ"] = [index[last.split()[1]]]
        elif op.startswith("s_cbranch"):
            b["succ"] = [index[last.split()[1]]] + nxt
        elif op == "s_endpgm":
            b["succ"] = []
        else:
            b["succ"] = nxt
    return blocks


def vregs(text):
    """the VGPR numbers an instruction names"""
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r"\bv(\d+)\b", text))
    return out


def gather_of(block):
    """(index of the last of the four loads, gathered registers) of a gather site, else None"""
    by_addr = {}
    for i, s in enumerate(block["ins"]):
        m = re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\], (.*?)(?: offset:(\d+))?$", s)
        if m:
            by_addr.setdefault(m.group(3), {})[int(m.group(4) or 0)] = (i, range(int(m.group(1)), int(m.group(2)) + 1))
    for loads in by_addr.values():
        if set(loads) >= {0, 16, 32, 48}:
            return max(loads[o][0] for o in (0, 16, 32, 48)), set().union(*(loads[o][1] for o in (0, 16, 32, 48)))
    return None


def reach(blocks, starts, stop, backwards=False):
    if backwards:
        edges = [[] for _ in blocks]
        for i, b in enumerate(blocks):
            for j in b["succ"]:
                edges[j].append(i)
    else:
        edges = [b["succ"] for b in blocks]
    seen, todo = set(), [s for s in starts if s not in stop]
    while todo:
        i = todo.pop()
        if i in seen:
            continue
        seen.add(i)
        todo.extend(j for j in edges[i] if j not in stop and j not in seen)
    return seen


def sites(lines):
    """one record per gather site of a kernel"""
    blocks = blocks_of(lines)
    gathers = {i: gather_of(b) for i, b in enumerate(blocks) if gather_of(b)}
    stop = set(gathers)
    for g in gathers:                                                  # the guard: falls into the site, and branches round it when no lane gathers
        if g > 0 and blocks[g - 1]["ins"] and blocks[g - 1]["ins"][-1].startswith("s_cbranch_execz") and g in blocks[g - 1]["succ"]:
            stop.add(g - 1)
    entry_blocks = {i for i, b in enumerate(blocks) if any(s.startswith("ds_read_b128") for s in b["ins"])}
    before_entries = reach(blocks, entry_blocks - stop, stop, backwards=True)
    out = []
    for g, (last, regs) in sorted(gathers.items()):
        region = reach(blocks, blocks[g]["succ"], stop) & before_entries
        text = (blocks[g]["ins"][last + 1:] if region else []) + [s for i in sorted(region) for s in blocks[i]["ins"]]
        waits = sum(1 for s in text if s.startswith("s_waitcnt") and "vmcnt" in s)
        named = [s for s in text if vregs(s) & regs]
        moves = sum(1 for s in named if s.startswith("v_mov"))
        out.append({"block": blocks[g]["name"], "regs": regs, "nblocks": len(region), "nins": len(text), "loops": len(region & entry_blocks),
                    "waits": waits, "moves": moves, "other": len(named) - moves})
    return out


def tuples(regs):
    r, out = sorted(regs), []
    for v in r:
        if out and out[-1][1] == v - 1:
            out[-1][1] = v
        else:
            out.append([v, v])
    return " ".join("v[%d:%d]" % (a, b) if a != b else "v%d" % a for a, b in out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", help="git revision whose gs_composite.hip is compiled (default: the working tree)")
    ap.add_argument("--same-as", help="git revision to compare the code of every kernel against (tools/isa_same.py)")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="gather_wait_")
    asm, regs = compile_asm(a.rev, os.path.join(tmp, "new.s"))
    print("# gs_composite.hip of %s, hipcc %s" % (a.rev or "the working tree", " ".join(FLAGS)))
    bad = 0
    for name, lines in kernel_bodies(asm).items():
        nice = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("(GsCompositeArgs)", "").replace("void ", "")
        r = regs.get(name, {})
        print("%-62s vgpr %3d spill %d scratch %3d occ %d" % (nice, r.get("VGPRs", -1), r.get("VGPRs Spill", -1), r.get("ScratchSize [bytes/lane]", -1),
                                                               r.get("Occupancy [waves/SIMD]", -1)))
        for s in sites(lines):
            if s["nblocks"]:
                bad += bool(s["waits"] or s["moves"] or s["other"])
                print("    gather %-10s -> %-37s region %3d blocks (%d per-entry) %4d instr: vmcnt waits %d, v_mov of gathered %d, other %d"
                      % (s["block"], tuples(s["regs"]), s["nblocks"], s["loops"], s["nins"], s["waits"], s["moves"], s["other"]))
            else:
                print("    gather %-10s -> %-37s region   0 blocks (feeds the staging directly)" % (s["block"], tuples(s["regs"])))
    print("# %d gather sites wait for, or touch, the gathered rows before the per-entry loops are over" % bad)
    if a.same_as:
        old, _ = compile_asm(a.same_as, os.path.join(tmp, "old.s"))
        print("# tools/isa_same.py: %s (parent) against %s" % (a.same_as, a.rev or "the working tree"))
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.join(ROOT, "tools/isa_same.py"), old, asm])


if __name__ == "__main__":
    main()
