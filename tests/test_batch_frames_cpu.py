"""The batch decode call's host side, without a device: the C entry point's call-level checks and the Python wrapper's
argument checks (dtype, shape, n+1 offsets, room for the records)."""
import ctypes

import pytest
import torch

from lz4_frame_conduit_amd import _ffi
from lz4_frame_conduit_amd.device import _check_batch_args
from lz4_frame_conduit_amd._ffi import Result

REC = ctypes.sizeof(Result)


def test_record_is_32_bytes():
    assert REC == 32


def test_null_engine_is_a_call_error():
    L = _ffi.lib()
    off = (ctypes.c_uint64 * 2)(0, 0)
    r = L.lz4f_mi355x_dev_decompressFrames(None, 1, None, 0, off, None, 0, off, None)
    assert L.LZ4F_isError(r)
    r = L.lz4f_mi355x_dev_decompressFrames(None, 0, None, 0, None, None, 0, None, None)
    assert L.LZ4F_isError(r)


def _args(n=3, **kw):
    a = dict(src=torch.zeros(100, dtype=torch.uint8), src_off=torch.zeros(n + 1, dtype=torch.int64), dst=torch.zeros(100, dtype=torch.uint8),
             dst_off=torch.zeros(n + 1, dtype=torch.int64), results=torch.zeros(n * REC, dtype=torch.uint8))
    a.update(kw)
    return a


def _check(**a):
    return _check_batch_args(a["src"], a["src_off"], a["dst"], a["dst_off"], a["results"], REC)


@pytest.mark.parametrize("bad, msg", [
    (dict(src=torch.zeros(100, dtype=torch.int8)), "src must be torch.uint8"),
    (dict(dst=torch.zeros(100, dtype=torch.float32)), "dst must be torch.uint8"),
    (dict(src_off=torch.zeros(4, dtype=torch.int32)), "src_off must be torch.int64"),
    (dict(dst_off=torch.zeros(4, dtype=torch.uint8)), "dst_off must be torch.int64"),
    (dict(results=torch.zeros(96, dtype=torch.int32)), "results must be torch.uint8"),
    (dict(src=torch.zeros(10, 10, dtype=torch.uint8)), "contiguous 1-d"),
    (dict(dst_off=torch.zeros(8, dtype=torch.int64)[::2]), "contiguous 1-d"),
    (dict(src_off=torch.zeros(0, dtype=torch.int64), dst_off=torch.zeros(0, dtype=torch.int64)), "n\\+1 offsets"),
    (dict(dst_off=torch.zeros(3, dtype=torch.int64)), "n\\+1 offsets"),
    (dict(results=torch.zeros(3 * 32 - 1, dtype=torch.uint8)), "results must hold 96 bytes for 3 frames"),
    (dict(src=[0] * 100), "src must be a tensor"),
])
def test_wrapper_rejects(bad, msg):
    with pytest.raises(ValueError, match=msg):
        _check(**_args(**bad))


def test_wrapper_wants_device_memory():
    # (everything else about these tensors is right: what is left is that they are host tensors)
    with pytest.raises(ValueError, match="device memory"):
        _check(**_args())
    with pytest.raises(ValueError, match="device memory"):
        _check(**_args(n=0, results=torch.zeros(0, dtype=torch.uint8)))
