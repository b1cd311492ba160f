"""The dictionary set's C ABI, as far as it goes without a device: the six functions of "A SET OF DICTIONARIES" in
include/lz4f_mi355x.h are declared, exported and bound, its three constants have the values the kernels use, and the calls that need
no engine answer as the header says."""
import ctypes
import os
import re

import pytest

from lz4_frame_conduit_amd import _ffi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lz4f_mi355x_dev_createDictSet", "lz4f_mi355x_dev_freeDictSet", "lz4f_mi355x_dictset_count", "lz4f_mi355x_dev_resolveDictIDs",
           "lz4f_mi355x_dev_compressFrames_usingDictSet", "lz4f_mi355x_dev_decompressFrames_usingDictSet")
CONSTANTS = {"LZ4F_MI355X_DICT_NONE": 0xFFFFFFFF, "LZ4F_MI355X_DICT_UNKNOWN": 0xFFFFFFFE, "LZ4F_MI355X_PATH_DICT_UNKNOWN": 0x4000}


@pytest.fixture(scope="module")
def L():
    _ffi.build()
    return _ffi.lib()


@pytest.fixture(scope="module")
def hdr():
    return open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()


def test_header_declares_and_library_exports(L, hdr):
    declared = set(re.findall(r"^LZ4F_MI355X_API[^;(]*?\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", hdr, flags=re.M))
    assert re.search(r"typedef\s+struct\s+lz4f_mi355x_dictset\s+lz4f_mi355x_dictset\s*;", hdr)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s


def test_constants(hdr):
    for name, value in CONSTANTS.items():
        m = re.search(r"^#define\s+%s\s+(0x[0-9A-Fa-f]+)u\b" % name, hdr, flags=re.M)
        assert m, name
        assert int(m.group(1), 16) == value, name
    # the path bit is one no other path bit has
    others = {n: int(v, 16) for n, v in re.findall(r"^#define\s+(LZ4F_MI355X_PATH_[A-Z_]+)\s+(0x[0-9A-Fa-f]+)u\b", hdr, flags=re.M)
              if n != "LZ4F_MI355X_PATH_DICT_UNKNOWN"}
    assert len(others) >= 14 and all(v & 0x4000 == 0 for v in others.values()), others
    assert (device.DICT_NONE, device.DICT_UNKNOWN, device.PATH_DICT_UNKNOWN) == (0xFFFFFFFF, 0xFFFFFFFE, 0x4000)


def test_ffi_gives_argument_types(L):
    for s in SYMBOLS:
        assert s in _ffi.DECLARED_SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.lz4f_mi355x_dev_createDictSet.argtypes) == 5 and L.lz4f_mi355x_dev_createDictSet.restype is ctypes.c_size_t
    assert len(L.lz4f_mi355x_dev_freeDictSet.argtypes) == 1 and L.lz4f_mi355x_dev_freeDictSet.restype is ctypes.c_size_t
    assert len(L.lz4f_mi355x_dictset_count.argtypes) == 1 and L.lz4f_mi355x_dictset_count.restype is ctypes.c_uint32
    assert len(L.lz4f_mi355x_dev_resolveDictIDs.argtypes) == 7 and L.lz4f_mi355x_dev_resolveDictIDs.restype is ctypes.c_size_t
    # the one-dictionary calls' arguments with a set and the slots where those have a handle, or a pointer and a size
    assert list(L.lz4f_mi355x_dev_compressFrames_usingDictSet.argtypes) == list(L.lz4f_mi355x_dev_compressFrames_usingCDict.argtypes) + [ctypes.c_void_p]
    assert list(L.lz4f_mi355x_dev_decompressFrames_usingDictSet.argtypes) == list(L.lz4f_mi355x_dev_decompressFrames_usingDict.argtypes[:-2]) + [ctypes.c_void_p] * 2
    assert L.lz4f_mi355x_dev_compressFrames_usingDictSet.restype is ctypes.c_size_t
    assert L.lz4f_mi355x_dev_decompressFrames_usingDictSet.restype is ctypes.c_size_t


def test_free_and_count_of_null(L):
    assert L.lz4f_mi355x_dev_freeDictSet(None) == 0
    assert L.lz4f_mi355x_dictset_count(None) == 0


def _generic(L, r) -> bool:
    return bool(L.LZ4F_isError(r)) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"


def test_create_without_engine_fails_and_says_why(L):
    out = ctypes.c_void_p(0xDEAD)
    assert _generic(L, L.lz4f_mi355x_dev_createDictSet(None, ctypes.byref(out), 0, None, None))
    assert not out.value, "*out must be NULL after a failed create"
    assert b"createDictSet" in L.lz4f_mi355x_last_error()
    # with members too; and a null `out` is an error that must not be written through
    hs, ids = (ctypes.c_void_p * 2)(None, None), (ctypes.c_uint32 * 2)(1, 2)
    out = ctypes.c_void_p(0xDEAD)
    assert _generic(L, L.lz4f_mi355x_dev_createDictSet(None, ctypes.byref(out), 2, hs, ids))
    assert not out.value
    assert _generic(L, L.lz4f_mi355x_dev_createDictSet(None, None, 0, None, None))


def test_calls_without_engine_fail(L):
    assert _generic(L, L.lz4f_mi355x_dev_resolveDictIDs(None, 1, None, 0, None, None, None))
    assert _generic(L, L.lz4f_mi355x_dev_compressFrames_usingDictSet(None, 1, None, 0, None, None, 0, None, None, None, None, None))
    assert _generic(L, L.lz4f_mi355x_dev_decompressFrames_usingDictSet(None, 1, None, 0, None, None, 0, None, None, None, None))
    assert _generic(L, L.lz4f_mi355x_dev_compressFrames_usingDictSet(None, 0, None, 0, None, None, 0, None, None, None, None, None))
