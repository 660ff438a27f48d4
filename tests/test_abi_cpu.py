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


def test_integration_doc_names_only_declared_symbols():
    """Every fer_* identifier INTEGRATION.md names is declared in include/fervit.h."""
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    known = set(re.findall(r"\bfer_[a-z0-9_]+", hdr))
    named = set(re.findall(r"\bfer_[a-z0-9_]+", open(os.path.join(ROOT, "INTEGRATION.md")).read()))
    assert named and not sorted(named - known), sorted(named - known)
