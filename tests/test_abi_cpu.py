"""CPU checks of the C ABI: the built library loads and exports every symbol that
include/fervit.h declares (no compute calls — there is no GPU here), and the ctypes
signature table and struct mirrors agree with the header's prototypes and structs, position by position."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fervit.h")
LIB = os.path.join(ROOT, "fer-vit_amd", "fervit", "libfervit.so")


def header():
    """include/fervit.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def declared():
    return sorted(set(re.findall(r"\b(fer_[a-z0-9_]+)\s*\(", header())))


# ---------------------------------------------------------------------- the header, parsed
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "fer_stream_t": ctypes.c_void_p}
STRUCT_RE = r"typedef\s+struct\s*\{(.*?)\}\s*(fer_[a-z0-9_]+)\s*;"
DECL_RE = r"(?:const\s+)?(\w+)\s*(\**)\s*(\w+)"  # [const] base [*...] name


def header_structs():
    """{struct name: [(field, base type, pointer depth)]} for every `typedef struct { ... } fer_*;`. A field
    declaration that does not read as `[const] type [*] name[, name ...]` raises."""
    out = {}
    for body, name in re.findall(STRUCT_RE, header(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = (p.strip() for p in decl.split(","))
            m = re.fullmatch(DECL_RE, first)
            assert m and all(re.fullmatch(r"\w+", n) for n in more), f"{name}: unreadable field declaration {decl!r}"
            fields += [(n, m.group(1), len(m.group(2))) for n in (m.group(3), *more)]
        out[name] = fields
    return out


def header_prototypes():
    """{entry point: (return (base, pointer depth), [(parameter, base, pointer depth)])}. Every statement of
    the header that names fer_*( must read as a prototype; one that does not raises."""
    src = re.sub(STRUCT_RE, "", header(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M).replace('extern "C" {', "")
    out = {}
    for stmt in (s.strip() for s in src.split(";")):
        if not re.search(r"\bfer_[a-z0-9_]+\s*\(", stmt):
            continue
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)\s*(fer_[a-z0-9_]+)\s*\(([^()]*)\)", stmt, flags=re.S)
        assert m, f"unreadable prototype {stmt!r}"
        params = []
        if m.group(4).strip() != "void":
            for p in m.group(4).split(","):
                pm = re.fullmatch(DECL_RE, " ".join(p.split()))
                assert pm, f"{m.group(3)}: unreadable parameter {p.strip()!r}"
                params.append((pm.group(3), pm.group(1), len(pm.group(2))))
        assert m.group(3) not in out, f"{m.group(3)} declared twice"
        out[m.group(3)] = ((m.group(1), len(m.group(2))), params)
    return out


def is_pointer_type(t):
    return isinstance(t, type) and issubclass(t, ctypes._Pointer)


def type_mismatch(base, depth, ct, mirrors):
    """None when ctypes type `ct` carries the C type `base` + depth stars, else what the header says."""
    c_name = base + "*" * depth
    if depth == 0:
        assert base in SCALARS, f"no ctypes counterpart known for the header's {base!r}"
        return None if ct is SCALARS[base] else c_name
    if ct in (ctypes.c_void_p, ctypes.c_char_p):
        return None
    if not is_pointer_type(ct):
        return c_name
    # a typed pointer says what it points to: the mirror of the header's struct, or its scalar
    pointee = (mirrors.get(base) or SCALARS.get(base)) if depth == 1 else None
    return None if pointee is not None and ct._type_ is pointee else c_name


def natural_layout(fields):
    """(offsets, size) of scalar / pointer fields under natural alignment (each at a multiple of its size)."""
    offs, off, align = [], 0, 1
    for _, base, depth in fields:
        n = 8 if depth else ctypes.sizeof(SCALARS[base])
        off = -(-off // n) * n
        offs.append(off)
        off, align = off + n, max(align, n)
    return offs, -(-off // align) * align


def test_header_declares_entry_points():
    names = declared()
    for n in ("fer_gemm", "fer_layernorm_fwd", "fer_layernorm_bwd", "fer_attention_fwd", "fer_attention_bwd",
              "fer_adamw", "fer_cross_entropy", "fer_wplus_fwd", "fer_decompose", "fer_last_error"):
        assert n in names


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.fer_version and ctypes.cast(lib.fer_last_error, ctypes.c_void_p).value


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built")
def test_ctypes_table_matches_header():
    """fervit/_lib.py against include/fervit.h: the same entry points; per entry point the same return
    type, parameter count and, position by position, kind and width; per mirrored struct the same fields
    in the same order with the same types, offsets and size. Every prototype and every struct of the header
    is covered: one the parser cannot read fails here."""
    from fervit import _lib
    from fervit._lib import SIGNATURES, lib

    L = lib()
    assert set(SIGNATURES) == set(declared())
    assert L.fer_version().decode().startswith("fervit")

    mirrors = {"fer_gemm_desc": _lib.GemmDesc, "fer_epilogue": _lib.Epilogue, "fer_wgrad_item": _lib.WgradItem,
               "fer_adamw_segment": _lib.AdamWSegment, "fer_image_aug": _lib.ImageAug}
    structs = header_structs()
    assert set(structs) == set(mirrors)
    in_lib = {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)
              and v is not ctypes.Structure}
    assert in_lib == set(mirrors.values()), "a ctypes.Structure of _lib.py has no struct of the header behind it"
    bad = []
    for name, fields in structs.items():
        S = mirrors[name]
        if [f for f, _, _ in fields] != [f for f, _ in S._fields_]:
            bad.append(f"{name}: field order: header {[f for f, _, _ in fields]}, {S.__name__} {[f for f, _ in S._fields_]}")
            continue
        offs, size = natural_layout(fields)
        for (f, base, depth), (_, ct), off in zip(fields, S._fields_, offs):
            want = type_mismatch(base, depth, ct, mirrors)
            if want:
                bad.append(f"{name}.{f}: header {want}, {S.__name__} {ct.__name__}")
            elif getattr(S, f).offset != off:
                bad.append(f"{name}.{f}: offset {off} in C, {getattr(S, f).offset} in {S.__name__}")
        if ctypes.sizeof(S) != size:
            bad.append(f"{name}: sizeof {size} in C, {ctypes.sizeof(S)} in {S.__name__}")

    protos = header_prototypes()
    assert set(protos) == set(SIGNATURES)
    returns = {("int", 0): ctypes.c_int, ("int64_t", 0): ctypes.c_int64, ("char", 1): ctypes.c_char_p}
    for name, (ret, params) in protos.items():
        res, args = SIGNATURES[name]
        assert ret in returns, f"{name}: no ctypes counterpart known for its return type {ret}"
        if res is not returns[ret]:
            bad.append(f"{name}: returns {ret[0] + '*' * ret[1]}, table {res.__name__}")
        if len(params) != len(args):
            bad.append(f"{name}: {len(params)} parameters in the header, {len(args)} in the table")
            continue
        for i, ((p, base, depth), ct) in enumerate(zip(params, args)):
            want = type_mismatch(base, depth, ct, mirrors)
            if want:
                bad.append(f"{name} argument {i} ({p}): header {want}, table {ct.__name__}")
    assert not bad, "\n".join(["fervit/_lib.py disagrees with include/fervit.h:"] + bad)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built")
def test_gemm_set_config_accepts_only_the_kept_configurations():
    """fer_gemm_set_config takes -1 (automatic) and the four tile configurations the library still
    has; every removed or unknown number is an error with a message (no GPU call involved)."""
    lib = ctypes.CDLL(LIB)
    lib.fer_gemm_set_config.argtypes = [ctypes.c_int]
    lib.fer_gemm_set_config.restype = ctypes.c_int
    lib.fer_last_error.restype = ctypes.c_char_p
    try:
        for cfg in (0, 1, 2, 4, 6, 7, 9, 10, 12, -2):
            assert lib.fer_gemm_set_config(cfg) != 0, cfg
            assert lib.fer_last_error(), cfg
        for cfg in (3, 5, 8, 11, -1):
            assert lib.fer_gemm_set_config(cfg) == 0, cfg
    finally:
        lib.fer_gemm_set_config(-1)


def dtype_entries():
    """Entry points whose first parameter is the dtype code (include/fervit.h spells it `int dtype`)."""
    return sorted(set(re.findall(r"\b(fer_[a-z0-9_]+)\s*\(\s*int\s+dtype\b", header())))


def zero_args(argtypes, dtype, **over):
    """dtype first, every other argument zero / null; `over` sets arguments by position."""
    args = [None if t is ctypes.c_void_p else (0.0 if t is ctypes.c_float else 0) for t in argtypes]
    args[0] = dtype
    for pos, v in over.items():
        args[int(pos[1:])] = v
    return args


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built")
def test_unknown_dtype_is_an_error_in_every_entry_point():
    """dtype = 7 with every other argument zero or null: each entry point that takes a dtype (and fer_gemm
    through its descriptor) returns non-zero and names itself and `unknown dtype` in fer_last_error. The
    check is the entry point's first statement, ahead of the empty-shape returns and of every HIP call, so
    this needs no GPU. (Messages name the entry without its fer_ prefix, like every message of the library.)"""
    from fervit._lib import SIGNATURES, Epilogue, GemmDesc, lib

    L = lib()
    names = dtype_entries()
    assert len(names) >= 24 and all(SIGNATURES[n][1][0] is ctypes.c_int for n in names), names
    for n in names:
        L.fer_set_persistent_mode(0)  # a success does not clear the message: every entry must write its own
        rc = getattr(L, n)(*zero_args(SIGNATURES[n][1], 7))
        msg = L.fer_last_error().decode()
        assert rc != 0 and "unknown dtype" in msg and msg.startswith(n[len("fer_"):] + ":"), (n, rc, msg)
    d, e = GemmDesc(), Epilogue()
    d.dtype = 7
    rc = L.fer_gemm(ctypes.byref(d), ctypes.byref(e), None)
    assert rc != 0 and L.fer_last_error().decode() == "gemm: unknown dtype"


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built")
@pytest.mark.parametrize("dtype", [0, 1])
def test_valid_dtype_with_an_empty_shape_still_returns_zero(dtype):
    """The entry points with an empty-shape early return (M, B, N, n or the element count <= 0) keep
    returning 0 for both valid codes; the size queries return 0 bytes / words for all-zero shapes."""
    from fervit._lib import SIGNATURES, Epilogue, GemmDesc, lib

    L = lib()
    empty = ["fer_layernorm_fwd", "fer_layernorm_bwd", "fer_attention_fwd", "fer_attention_bwd", "fer_colsum",
             "fer_tokens_fwd", "fer_tokens_bwd", "fer_head_fwd", "fer_head_bwd", "fer_axpy", "fer_dropout",
             "fer_attention_ws", "fer_attention_saved_floats"]
    assert set(empty) <= set(dtype_entries())
    for n in empty:
        assert getattr(L, n)(*zero_args(SIGNATURES[n][1], dtype)) == 0, n
    # patch size 1 (the element count divides by it), still no elements
    assert L.fer_im2col_patch(*zero_args(SIGNATURES["fer_im2col_patch"][1], dtype, a6=1)) == 0
    d, e = GemmDesc(), Epilogue()
    d.dtype = dtype
    assert L.fer_gemm(ctypes.byref(d), ctypes.byref(e), None) == 0


def test_integration_doc_names_only_declared_symbols():
    """Every fer_* identifier INTEGRATION.md names is declared in include/fervit.h, or, where the text
    calls it as a method (`.fer_*(`), is a method of FerModule."""
    from fervit.module import FerModule

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    methods = {n for n in re.findall(r"\.(fer_[a-z0-9_]+)\(", doc) if callable(getattr(FerModule, n, None))}
    known = set(re.findall(r"\bfer_[a-z0-9_]+", header()))
    named = set(re.findall(r"\bfer_[a-z0-9_]+", doc)) - methods
    assert named and not sorted(named - known), sorted(named - known)
