"""CPU checks of the C ABI: the built library loads and exports every symbol that
include/fervit.h declares (no compute calls — there is no GPU here), and the ctypes
signature table covers exactly that set."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fervit.h")
LIB = os.path.join(ROOT, "fer-vit_amd", "fervit", "libfervit.so")


def declared():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fer_[a-z0-9_]+)\s*\(", src)))


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
    from fervit._lib import SIGNATURES, lib

    L = lib()
    assert set(SIGNATURES) == set(declared())
    assert L.fer_version().decode().startswith("fervit")


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
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fer_[a-z0-9_]+)\s*\(\s*int\s+dtype\b", src)))


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
    """Every fer_* identifier INTEGRATION.md names is declared in include/fervit.h."""
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    known = set(re.findall(r"\bfer_[a-z0-9_]+", hdr))
    named = set(re.findall(r"\bfer_[a-z0-9_]+", open(os.path.join(ROOT, "INTEGRATION.md")).read()))
    assert named and not sorted(named - known), sorted(named - known)
