"""The C-ABI library loads and exports every symbol include/gsplat.h declares, and the ctypes binding states the header's ABI: the
table of signatures, the four structures and every integer constant of gaussiansplat_amd/backend.py, and the constants of
julia/backend.jl, each against the header's text (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

import abi_header as H
from abi_header import ROOT


@pytest.fixture(scope="module")
def lib():
    from gaussiansplat_amd import build
    build.build()
    from gaussiansplat_amd import backend
    return backend.load()


def _declared_functions():
    src = H._strip_comments(open(H.HEADER).read())
    return sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    from gaussiansplat_amd import backend
    names = _declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gsplat.h but not exported"
    assert sorted(backend.SYMBOLS) == names, "backend.SYMBOLS out of sync with include/gsplat.h"


def test_abi_version_and_config_layout(lib):
    from gaussiansplat_amd import backend
    assert lib.gs_abi_version() == backend.GS_ABI_VERSION == 3
    cfg = backend.default_config()
    assert cfg.struct_size == C.sizeof(backend.GsConfig) == 96 and cfg.abi_version == 3
    assert cfg.schedule == 3 and cfg.slab_mode == 1 and cfg.debug_flags == 0 and cfg.slab_max_ratio == 0.0 and cfg.list_cap == 0
    assert cfg.tile_parts == 0 and list(cfg.reserved) == [0, 0, 0]              # reserved words, and the one that got a name, default to 0
    hdr = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert re.search(r"#define GS_ABI_VERSION\s+3\b", hdr)
    assert cfg.tile_size == 16 and cfg.order == backend.ORDER_DEPTH_DESC and abs(cfg.t_min - 1e-5) < 1e-12


CSRC = os.path.join(ROOT, "gaussiansplat_amd", "csrc")
_PY_SCALAR = {None: "void", C.c_int32: "i32", C.c_int64: "i64", C.c_float: "f32", C.c_double: "f64"}        # (c_int is c_int32 here)
_PY_POINTEE = {C.c_float: "float", C.c_double: "double", C.c_int64: "int64_t", C.c_int32: "int32_t"}
_PY_STRUCTS = {"gs_config": "GsConfig", "gs_grads": "GsGrads", "gs_density_stats": "GsDensityStats", "gs_density_params": "GsDensityParams"}


def _py_kind(t):
    """(kind, pointee) of a ctypes restype / argtype, in the terms of abi_header._c_kind; pointee None: any pointer (c_void_p, c_char_p)."""
    from gaussiansplat_amd import backend
    if t in _PY_SCALAR:
        return _PY_SCALAR[t], None
    if t in (C.c_void_p, C.c_char_p):
        return "ptr", None
    assert isinstance(t, type) and issubclass(t, C._Pointer), f"unknown ctypes type {t!r}"
    inner = t._type_
    if inner is C.c_void_p:
        return "ptr", ("void", 2)
    structs = {getattr(backend, py): c for c, py in _PY_STRUCTS.items()}
    return "ptr", (structs[inner] if inner in structs else _PY_POINTEE[inner], 1)


def _py_compatible(ck, pk, name, what):
    kind_c, pt_c = ck
    kind_p, pt_p = pk
    assert kind_c == kind_p, f"{name}: {what}: C {ck} vs ctypes {pk}"
    if kind_c != "ptr" or pt_p is None:
        return
    base_c, n_c = pt_c
    base_p, n_p = pt_p
    assert n_c == n_p, f"{name}: {what}: pointer depth C {pt_c} vs ctypes {pt_p}"
    if base_c == "gs_ctx":
        assert base_p == "void", f"{name}: {what}: gs_ctx* must be c_void_p"
    elif base_c != "void":
        assert base_c == base_p, f"{name}: {what}: pointee C {base_c} vs ctypes {base_p}"


def test_table_matches_every_prototype(lib):
    """backend.ABI against include/gsplat.h: the same functions in the same order, and per function the arity, the scalar widths and,
    where ctypes names one, the pointee of every argument and of the return value."""
    from gaussiansplat_amd import backend
    protos = H._c_prototypes()
    assert len(protos) >= 80
    assert list(backend.ABI) == list(protos), "backend.ABI and the prototypes of include/gsplat.h differ in members or order"
    assert backend.SYMBOLS == tuple(backend.ABI)
    for name, (cret, cargs) in protos.items():
        sig = backend.ABI[name]
        assert len(sig.argtypes) == len(cargs), f"{name}: {len(sig.argtypes)} argtypes, prototype has {len(cargs)}"
        _py_compatible(H._c_kind(cret), _py_kind(sig.restype), name, "return")
        for k, (ca, pt) in enumerate(zip(cargs, sig.argtypes)):
            _py_compatible(H._c_kind(ca), _py_kind(pt), name, f"argument {k} ({ca})")
        if hasattr(lib, name):                                  # what load() applied is the table
            f = getattr(lib, name)
            assert f.restype is sig.restype and list(f.argtypes) == list(sig.argtypes), name
    assert [n for n, s in backend.ABI.items() if s.optional] == ["gs_debug_tail_fill"]


def test_structures_mirror_the_header(lib):
    from gaussiansplat_amd import backend
    scalar = {"int32_t": (C.c_int32, 4), "float": (C.c_float, 4)}
    for cname, pyname in _PY_STRUCTS.items():
        cf, S = H._c_struct_fields(cname), getattr(backend, pyname)
        assert [f[0] for f in S._fields_] == [f[0] for f in cf], f"{pyname}: field names / order differ from {cname}"
        total = 0
        for (fname, ctype, cnt), (_, ptype) in zip(cf, S._fields_):
            if ctype.endswith("*"):
                want, size = C.c_void_p, 8
            else:
                want, size = scalar[ctype]
            if cnt > 1:
                assert issubclass(ptype, C.Array) and ptype._type_ is want and ptype._length_ == cnt, f"{pyname}.{fname}: {ctype}[{cnt}]"
            else:
                assert ptype is want, f"{pyname}.{fname}: {ctype} vs {ptype}"
            total += size * cnt
        assert C.sizeof(S) == total, f"sizeof({pyname}) = {C.sizeof(S)}, the fields of {cname} add up to {total}"    # (no struct here needs padding)
    assert C.sizeof(backend.GsConfig) == 96 and C.sizeof(backend.GsGrads) == 40


# integer constants of backend.py that state no header's value, on purpose (none today: every one of them is the ABI's)
NOT_FROM_A_HEADER = ()


def test_python_constants_equal_the_headers(lib):
    """Every integer constant of backend.py equals the header value it states; one that is in no header and not listed above fails."""
    from gaussiansplat_amd import backend
    hdr = H._c_constants()
    want = {k: v for k, v in hdr.items() if k.startswith("GS_")}
    want["GS_EXPOSURE_FLOATS"] = H._c_constants(os.path.join(CSRC, "gs_exposure.h"))["GS_EXPOSURE_FLOATS"]
    want["KNN_BOX"] = H._c_constants(os.path.join(CSRC, "gs_knn.h"))["GS_KNN_BOX"]
    want["TOUCHED_CHUNK"] = H._c_constants(os.path.join(CSRC, "gs_chunk.h"))["GS_CHUNK"]
    for prefix in ("ORDER_", "ARR_", "METRIC_"):
        want.update({k[3:]: v for k, v in hdr.items() if k.startswith("GS_" + prefix)})
    ints = {k: v for k, v in vars(backend).items() if isinstance(v, int)}
    assert len(ints) >= 40
    for k, v in ints.items():
        if k in NOT_FROM_A_HEADER:
            continue
        assert k in want, f"backend.{k} = {v}: an integer constant that is in no header and not in NOT_FROM_A_HEADER"
        assert v == want[k], f"backend.{k} = {v}, the header says {want[k]}"
    for k in ("GS_BWD_OVERWRITE", "GS_BWD_COMPOSITE_ONLY", "GS_BWD_PARAMS_ONLY", "GS_BWD_PARAMS_SH", "GS_BWD_PARAMS_GEOM"):
        assert k in ints, k
    for prefix, enum in (("ORDER_", "gs_order"), ("ARR_", "gs_array")):                 # every enumerator has its Python name
        assert {k[3:] for k, _ in H._c_enum(enum)} == {k for k in ints if k.startswith(prefix)}, enum
    stages = H._c_enum("gs_stage")
    assert stages[-1] == ("GS_STAGE_COUNT", len(backend.STAGES)) and [v for _, v in stages] == list(range(len(stages)))
    assert tuple(k[len("GS_STAGE_"):].lower() for k, _ in stages[:-1]) == backend.STAGES


def test_julia_constants_equal_the_headers():
    """Every `const GS_X = ...` of julia/backend.jl states a value of include/gsplat.h (GS_EXPOSURE_FLOATS: of csrc/gs_exposure.h)."""
    want = dict(H._c_constants(os.path.join(CSRC, "gs_exposure.h")), **H._c_constants())
    src = re.sub(r"(?m)#.*$", "", open(os.path.join(ROOT, "julia", "backend.jl")).read())
    consts = re.findall(r"(?m)^const\s+(GS_[A-Z0-9_]+)\s*=\s*(.*?)\s*$", src)
    assert len(consts) >= 14
    for name, expr in consts:
        m = re.fullmatch(r"(?:Cint\()?(-?\d+)\)?", expr)
        assert m, f"julia/backend.jl: const {name} = {expr}: not an integer literal"
        assert name in want, f"julia/backend.jl: const {name} is in no header"
        assert int(m.group(1)) == want[name], f"julia/backend.jl: const {name} = {m.group(1)}, the header says {want[name]}"


def test_no_cpu_fallback(lib):
    """Without a HIP device the product path must fail loudly (never route through a CPU path)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gaussiansplat_amd import backend, renderer
    with pytest.raises(backend.GsError) as e:
        backend.Context()
    assert e.value.code == -2
    with pytest.raises(RuntimeError):
        renderer.getRenderer("GAUSSIAN_3D", (64, 64, 3), (16, 16), (4, 4), 100)


def test_product_never_imports_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    pkg = os.path.join(ROOT, "gaussiansplat_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "gs_oracle" not in txt, os.path.join(dp, f)
