"""The prepared dictionary's C ABI, as far as it goes without a device: lz4f_mi355x_dev_createCDict, lz4f_mi355x_dev_freeCDict,
lz4f_mi355x_cdict_data and lz4f_mi355x_dev_compressFrames_usingCDict are declared, exported and bound, and the calls that need no
engine answer as include/lz4f_mi355x.h says."""
import ctypes
import os
import re

import pytest

from lz4_frame_conduit_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lz4f_mi355x_dev_createCDict", "lz4f_mi355x_dev_freeCDict", "lz4f_mi355x_cdict_data", "lz4f_mi355x_dev_compressFrames_usingCDict")


@pytest.fixture(scope="module")
def L():
    _ffi.build()
    return _ffi.lib()


def test_header_declares_and_library_exports(L):
    hdr = open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()
    declared = set(re.findall(r"^LZ4F_MI355X_API[^;(]*?\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", hdr, flags=re.M))
    assert re.search(r"typedef\s+struct\s+lz4f_mi355x_cdict\s+lz4f_mi355x_cdict\s*;", hdr)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s


def test_ffi_gives_argument_types(L):
    for s in SYMBOLS:
        assert s in _ffi.DECLARED_SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.lz4f_mi355x_dev_createCDict.argtypes) == 4 and L.lz4f_mi355x_dev_createCDict.restype is ctypes.c_size_t
    assert len(L.lz4f_mi355x_dev_freeCDict.argtypes) == 1
    assert len(L.lz4f_mi355x_cdict_data.argtypes) == 2 and L.lz4f_mi355x_cdict_data.restype is ctypes.c_void_p
    # the _usingDict call's arguments with one handle where that has a pointer and a size
    using_dict = L.lz4f_mi355x_dev_compressFrames_usingDict.argtypes
    assert list(L.lz4f_mi355x_dev_compressFrames_usingCDict.argtypes) == list(using_dict[:-2]) + [ctypes.c_void_p]


def test_free_of_null_is_accepted(L):
    assert L.lz4f_mi355x_dev_freeCDict(None) == 0


def test_create_without_engine_fails_and_says_why(L):
    out = ctypes.c_void_p(0xDEAD)
    r = L.lz4f_mi355x_dev_createCDict(None, ctypes.byref(out), None, 0)
    assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
    assert not out.value, "*out must be NULL after a failed create"
    assert b"createCDict" in L.lz4f_mi355x_last_error()
    # a null `out` is an error too, and must not be written through
    assert L.LZ4F_isError(L.lz4f_mi355x_dev_createCDict(None, None, None, 0))


def test_data_of_null_is_null_and_empty(L):
    n = ctypes.c_size_t(12345)
    assert L.lz4f_mi355x_cdict_data(None, ctypes.byref(n)) is None
    assert n.value == 0
    assert L.lz4f_mi355x_cdict_data(None, None) is None


def test_compress_without_engine_fails(L):
    assert L.LZ4F_isError(L.lz4f_mi355x_dev_compressFrames_usingCDict(None, 0, None, 0, None, None, 0, None, None, None, None))
