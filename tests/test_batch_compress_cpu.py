"""The batch encode call's host side, without a device: the exported symbol and its call-level checks, the Python wrapper's
argument checks, and the window-offset helper (cumulative lz4f_mi355x_compressFrameBound, a host function)."""
import ctypes
import os

import pytest
import torch

from lz4_frame_conduit_amd import _ffi, conduit, device
from lz4_frame_conduit_amd._ffi import Preferences, Result
from lz4_frame_conduit_amd.device import Engine

REC = ctypes.sizeof(Result)


def test_symbol_is_exported_and_declared():
    assert "lz4f_mi355x_dev_compressFrames" in _ffi.DECLARED_SYMBOLS
    L = _ffi.lib()
    assert L.lz4f_mi355x_dev_compressFrames.restype is ctypes.c_size_t
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_ffi.__file__))), "include", "lz4f_mi355x.h")) as f:
        assert "lz4f_mi355x_dev_compressFrames(" in f.read()


def test_null_engine_is_a_call_error():
    L = _ffi.lib()
    off = (ctypes.c_uint64 * 2)(0, 0)
    r = L.lz4f_mi355x_dev_compressFrames(None, 1, None, 0, off, None, 0, off, None, None)
    assert L.LZ4F_isError(r)
    r = L.lz4f_mi355x_dev_compressFrames(None, 0, None, 0, None, None, 0, None, None, None)
    assert L.LZ4F_isError(r)


def _engine_without_device():
    """An Engine that was never opened: the wrapper's checks come before anything that needs one."""
    e = Engine.__new__(Engine)
    e.h = None
    return e


def _args(n=3, **kw):
    a = dict(src=torch.zeros(100, dtype=torch.uint8), src_off=torch.zeros(n + 1, dtype=torch.int64), dst=torch.zeros(100, dtype=torch.uint8),
             dst_off=torch.zeros(n + 1, dtype=torch.int64), prefs=conduit.make_preferences(blockSizeID=4), results=torch.zeros(n * REC, dtype=torch.uint8))
    a.update(kw)
    return a


def _call(**a):
    return _engine_without_device().compress_frames_async(a["src"], a["src_off"], a["dst"], a["dst_off"], a["prefs"], a["results"])


@pytest.mark.parametrize("bad, msg", [
    (dict(src=torch.zeros(100, dtype=torch.int8)), "src must be torch.uint8"),
    (dict(dst=torch.zeros(100, dtype=torch.float32)), "dst must be torch.uint8"),
    (dict(src_off=torch.zeros(4, dtype=torch.int32)), "src_off must be torch.int64"),
    (dict(dst_off=torch.zeros(4, dtype=torch.uint8)), "dst_off must be torch.int64"),
    (dict(results=torch.zeros(96, dtype=torch.int32)), "results must be torch.uint8"),
    (dict(src=torch.zeros(10, 10, dtype=torch.uint8)), "contiguous 1-d"),
    (dict(src_off=torch.zeros(0, dtype=torch.int64), dst_off=torch.zeros(0, dtype=torch.int64)), "n\\+1 offsets"),
    (dict(dst_off=torch.zeros(3, dtype=torch.int64)), "n\\+1 offsets"),
    (dict(results=torch.zeros(3 * 32 - 1, dtype=torch.uint8)), "results must hold 96 bytes for 3 frames"),
    (dict(src=[0] * 100), "src must be a tensor"),
    (dict(prefs=None), "prefs must be a Preferences"),
    (dict(prefs={"blockSizeID": 4}), "prefs must be a Preferences"),
    (dict(prefs=conduit.make_preferences().frameInfo), "prefs must be a Preferences"),
])
def test_wrapper_rejects(bad, msg):
    with pytest.raises(ValueError, match=msg):
        _call(**_args(**bad))


def test_wrapper_wants_device_memory():
    # (everything else about these tensors is right: what is left is that they are host tensors)
    with pytest.raises(ValueError, match="device memory"):
        _call(**_args())
    with pytest.raises(ValueError, match="device memory"):
        _call(**_args(n=0, results=torch.zeros(0, dtype=torch.uint8)))


@pytest.mark.parametrize("kw", [dict(blockSizeID=4), dict(blockSizeID=5, blockChecksum=1), dict(blockSizeID=7, contentChecksum=1, contentSize=1),
                                dict(blockSizeID=6, blockChecksum=1, contentChecksum=1, dictID=9, blockMode=0), dict()])
def test_window_offsets_are_cumulative_bounds(kw):
    L = _ffi.lib()
    p = conduit.make_preferences(**kw)
    lens = [0, 1, 4, 65535, 65536, 65537, (256 << 10) - 1, 256 << 10, (1 << 20) + 1, 5 << 20, 0, 123]
    bounds = [L.lz4f_mi355x_compressFrameBound(n, ctypes.byref(p)) for n in lens]
    assert not any(L.LZ4F_isError(b) for b in bounds)
    for gap in (0, 1, 192):
        offs = device.frame_windows(lens, p, gap)
        assert len(offs) == len(lens) + 1 and offs[0] == 0
        assert [offs[i + 1] - offs[i] for i in range(len(lens))] == [b + gap for b in bounds]
    assert device.frame_windows([], p) == [0]


def test_window_offsets_reject_what_has_no_bound():
    with pytest.raises(ValueError, match="prefs must be a Preferences"):
        device.frame_windows([1, 2], None)
    with pytest.raises(ValueError, match="gap"):
        device.frame_windows([1, 2], conduit.make_preferences(), -1)
    bad = Preferences()
    bad.frameInfo.blockSizeID = 3
    with pytest.raises(device.DeviceCodecError, match="maxBlockSize_invalid"):
        device.frame_windows([1], bad)
