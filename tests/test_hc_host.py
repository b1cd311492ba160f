"""Compression levels 3-12 on the host side (no GPU needed): the level reaches the ABI, the bound does not depend on it, and a
high level without a device fails loudly like level 0 does - there is no CPU fallback at any level."""
import ctypes

import pytest

from lz4_frame_conduit_amd import _ffi, conduit


@pytest.fixture(scope="module")
def L():
    return _ffi.lib()


def test_make_preferences_writes_the_level_at_its_abi_offset():
    p = conduit.make_preferences(blockSizeID=7, blockMode=1, compressionLevel=9)
    raw = bytes(memoryview(p))
    off = _ffi.Preferences.compressionLevel.offset
    assert off == 32 and ctypes.sizeof(_ffi.Preferences) == 56          # LZ4F_preferences_t: frameInfo (32 bytes), then the level
    assert int.from_bytes(raw[off:off + 4], "little", signed=True) == 9
    assert conduit.make_preferences().compressionLevel == 0
    assert int.from_bytes(bytes(memoryview(conduit.make_preferences(compressionLevel=-3)))[off:off + 4], "little", signed=True) == -3


def test_compress_bound_does_not_depend_on_the_level(L):
    for n in (0, 1, 65535, 65536, 5 << 20):
        for kw in (dict(blockSizeID=4, blockMode=0), dict(blockSizeID=7, blockMode=1, blockChecksum=1, contentChecksum=1)):
            for auto in (0, 1):
                b0 = L.LZ4F_compressBound(n, ctypes.byref(conduit.make_preferences(autoFlush=auto, **kw)))
                for lvl in (3, 9, 12, 16):
                    assert L.LZ4F_compressBound(n, ctypes.byref(conduit.make_preferences(autoFlush=auto, compressionLevel=lvl, **kw))) == b0
                assert L.lz4f_mi355x_compressFrameBound(n, ctypes.byref(conduit.make_preferences(compressionLevel=9, **kw))) == \
                    L.lz4f_mi355x_compressFrameBound(n, ctypes.byref(conduit.make_preferences(**kw)))


def test_high_level_without_device_fails_loudly(L):
    """Level 9 is accepted (no ERROR_compressionLevel_invalid any more) and, without a device, fails where level 0 fails."""
    if L.lz4f_mi355x_device_count() > 0:
        pytest.skip("a GPU is present")
    p = conduit.make_preferences(blockSizeID=4, compressionLevel=9)
    with pytest.raises(conduit.Lz4FrameError, match="lz4frame error: ERROR_GENERIC"):
        conduit.compressWithPreferences(p, [b"x" * 70000])
    assert b"no usable HIP device" in L.lz4f_mi355x_last_error()
    data = b"y" * 100000
    cap = L.lz4f_mi355x_compressFrameBound(len(data), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    r = L.lz4f_mi355x_compressFrame(dst, cap, data, len(data), ctypes.byref(p))
    assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
    with pytest.raises(conduit.Lz4FrameError):
        conduit.compressBatched([data], p)
    # the streaming API: the header is host work, the first block needs the device
    c = ctypes.c_void_p()
    assert L.LZ4F_createCompressionContext(ctypes.byref(c), 100) == 0
    hdr = ctypes.create_string_buffer(32)
    assert not L.LZ4F_isError(L.LZ4F_compressBegin(c, hdr, 32, ctypes.byref(p)))
    bound = L.LZ4F_compressBound(len(data), ctypes.byref(p))
    out = ctypes.create_string_buffer(bound)
    r = L.LZ4F_compressUpdate(c, out, bound, data, len(data), None)
    assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
    L.LZ4F_freeCompressionContext(c)
