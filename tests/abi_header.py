"""include/gsplat.h read as text: prototypes, struct fields, #define'd integers and enumerators.

The one header reader of the tests that tie a statement of the C ABI to the header (tests/test_abi.py: the ctypes table, structures
and constants of gaussiansplat_amd/backend.py; tests/test_julia_glue.py: the ccalls, structs and constants of julia/backend.jl) and
of tools/build_old_lib.sh, which writes its stubs from the prototypes.  Plain regular expressions over the header's own style, no C parser.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat.h")


def _strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _c_prototypes(path=HEADER):
    src = _strip_comments(open(path).read())
    protos = {}
    for m in re.finditer(r"(?m)^\s*((?:const\s+)?[A-Za-z_0-9]+\s*\**)\s*(gs_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        alist = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
        protos[name] = (ret, alist)
    return protos


def _c_kind(decl):
    """(kind, pointee) of a C parameter / return declaration."""
    d = re.sub(r"\bconst\b", "", decl).strip()
    arr = "[" in d
    d = re.sub(r"\[.*?\]", "", d).strip()
    stars = d.count("*")
    d = d.replace("*", " ").split()
    base = d[0] if d else ""
    if len(d) > 1 and d[0] in ("unsigned", "long"):
        base = " ".join(d[:-1])
    nptr = stars + (1 if arr else 0)
    if nptr == 0:
        return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "f32", "double": "f64", "void": "void"}[base], None
    return "ptr" * 1, (base, nptr)


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "({[":
            depth += 1
        elif ch in ")}]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return [x.strip() for x in out]


def _c_struct_fields(name):
    src = _strip_comments(open(HEADER).read())
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", src)
    fields = []
    for line in m.group(1).split(";"):
        line = line.strip()
        if not line:
            continue
        fm = re.fullmatch(r"([A-Za-z_0-9]+)\s*(\*?)\s*([A-Za-z_0-9]+)(?:\[(\d+)\])?", line)
        assert fm, line
        fields.append((fm.group(3), fm.group(1) + fm.group(2), int(fm.group(4) or 1)))
    return fields


def _c_enums(path=HEADER):
    """[(type name or "", [(enumerator, value), ...]), ...] of a header; an enumerator without '= n' is its predecessor + 1 (the first: 0)."""
    src = re.sub(r"//.*", "", _strip_comments(open(path).read()))
    enums = []
    for m in re.finditer(r"\benum\s*\{([^}]*)\}\s*([A-Za-z_0-9]*)\s*;", src):
        items, nxt = [], 0
        for e in m.group(1).split(","):
            e = e.strip()
            if not e:
                continue
            em = re.fullmatch(r"([A-Za-z_0-9]+)(?:\s*=\s*(-?\d+))?", e)
            assert em, e
            val = nxt if em.group(2) is None else int(em.group(2))
            items.append((em.group(1), val))
            nxt = val + 1
        enums.append((m.group(2), items))
    return enums


def _c_enum(name, path=HEADER):
    """The enumerators of `typedef enum { ... } name;` as [(enumerator, value), ...] in the header's order."""
    found = [items for n, items in _c_enums(path) if n == name]
    assert len(found) == 1, name
    return found[0]


def _c_constants(path=HEADER):
    """{name: value} of every `#define NAME <integer>` and every enumerator of a header."""
    src = re.sub(r"//.*", "", _strip_comments(open(path).read()))
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"(?m)^[ \t]*#[ \t]*define[ \t]+([A-Za-z_0-9]+)[ \t]+(-?\d+)[ \t]*$", src)}
    for _, items in _c_enums(path):
        for k, v in items:
            assert k not in vals, k
            vals[k] = v
    return vals
