"""The C ABI of the prepared dictionary for levels 3-12, as far as it goes without a device: lz4f_mi355x_dev_createCDictHC and
lz4f_mi355x_cdict_has_hc are declared, exported and bound, and the calls that need no engine answer as include/lz4f_mi355x.h says."""
import ctypes
import os
import re

import pytest

from lz4_frame_conduit_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lz4f_mi355x_dev_createCDictHC", "lz4f_mi355x_cdict_has_hc")


@pytest.fixture(scope="module")
def L():
    _ffi.build()
    return _ffi.lib()


def test_header_declares_and_library_exports(L):
    hdr = open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()
    declared = set(re.findall(r"^LZ4F_MI355X_API[^;(]*?\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", hdr, flags=re.M))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s


def test_ffi_gives_argument_types(L):
    for s in SYMBOLS:
        assert s in _ffi.DECLARED_SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s
    # createCDict's argument list and result
    assert list(L.lz4f_mi355x_dev_createCDictHC.argtypes) == list(L.lz4f_mi355x_dev_createCDict.argtypes)
    assert L.lz4f_mi355x_dev_createCDictHC.restype is L.lz4f_mi355x_dev_createCDict.restype is ctypes.c_size_t
    assert list(L.lz4f_mi355x_cdict_has_hc.argtypes) == [ctypes.c_void_p] and L.lz4f_mi355x_cdict_has_hc.restype is ctypes.c_int


def test_header_gives_createCDictHC_the_arguments_of_createCDict():
    hdr = open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()
    args = {n: re.sub(r"\s+", " ", a).strip() for n, a in re.findall(r"^LZ4F_MI355X_API\s+size_t\s+(lz4f_mi355x_dev_createCDict(?:HC)?)\s*\(([^)]*)\)", hdr, flags=re.M)}
    assert args["lz4f_mi355x_dev_createCDictHC"] == args["lz4f_mi355x_dev_createCDict"]


def test_create_without_engine_fails_and_says_why(L):
    out = ctypes.c_void_p(0xDEAD)
    r = L.lz4f_mi355x_dev_createCDictHC(None, ctypes.byref(out), None, 0)
    assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
    assert not out.value, "*out must be NULL after a failed create"
    assert b"createCDictHC" in L.lz4f_mi355x_last_error()
    # a null `out` is an error too, and must not be written through
    assert L.LZ4F_isError(L.lz4f_mi355x_dev_createCDictHC(None, None, None, 0))


def test_has_hc_of_null_is_0(L):
    assert L.lz4f_mi355x_cdict_has_hc(None) == 0
