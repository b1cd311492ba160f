"""tests/pack_model.py held to the oracle, and the pack's host side held to the model: a packed stream, with and without its
directory, is a concatenated .lz4 stream that decodes frame after frame to the inputs in order; lz4f_mi355x_packDirectorySize and
lz4f_mi355x_peekPackDirectory say what the model says; the four symbols are declared, exported and bound; and the device calls
answer ERROR_GENERIC without an engine."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import oracle
import pack_model as pm
from lz4_frame_conduit_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lz4f_mi355x_dev_packFrames", "lz4f_mi355x_packDirectorySize", "lz4f_mi355x_peekPackDirectory", "lz4f_mi355x_dev_readPackDirectory")
SIZES = (0, 1, 12, 13, 4096, 70000)


@pytest.fixture(scope="module")
def L():
    _ffi.build()
    return _ffi.lib()


@pytest.fixture(scope="module")
def batch():
    """Windows as a compress call leaves them: frame i at the start of window i, stale bytes behind it; one slot failed."""
    rng = np.random.default_rng(11)
    inputs = []
    for n in SIZES:
        a = rng.integers(0, 256, n, dtype=np.uint8)
        a[n // 3:] = a[n // 3:] & 3                            # (something to compress)
        inputs.append(a.tobytes())
    frames = [oracle.conduit_compress(x) for x in inputs]
    inputs.append(inputs[4])
    frames.append(oracle.conduit_compress(inputs[4], oracle.mkprefs(bsid=4, indep=1, cck=1, bck=1)))
    src, src_off, records, want = bytearray(), [0], [], []
    for k, (x, f) in enumerate(zip(inputs, frames)):
        if k == 3:                                             # the failed slot: a window with rubbish in it, and a record that says so
            src += b"\xEE" * 40
            src_off.append(len(src))
            records.append((pm.ST_DSTSMALL, 0))
        src += f + b"\xEE" * (k % 3)
        src_off.append(len(src))
        records.append((0, len(f)))
        want.append(x)
    return bytes(src), src_off, records, want


def decode_stream(stream: bytes):
    """Frame after frame, stepping by `consumed` -> (the outputs of the LZ4 frames, the skippable frames' sizes)."""
    outs, skipped, pos = [], [], 0
    while pos < len(stream):
        magic = struct.unpack_from("<I", stream, pos)[0]
        out, used = oracle.decompress_frame(stream[pos:])
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            assert out == b""
            skipped.append(used)
        else:
            outs.append(out)
        assert used > 0
        pos += used
    assert pos == len(stream)
    return outs, skipped


@pytest.mark.parametrize("with_dir", [False, True])
def test_packed_stream_decodes_to_the_inputs_in_order(batch, with_dir):
    src, src_off, records, want = batch
    n = len(records)
    dst, dst_off, rec = pm.pack(src, src_off, records, 1 << 30, with_dir)
    D = pm.directory_size(n) if with_dir else 0
    assert rec == pm.Rec(0, len(dst), len(dst) - D, n - 1, pm.NONE, pm.PATH_BATCH)
    assert dst_off[0] == D and dst_off[-1] == len(dst) and dst_off[3] == dst_off[4]          # (the failed slot: an empty span)
    outs, skipped = decode_stream(dst)
    assert outs == want
    assert skipped == ([D] if with_dir else [])
    for i, (st, size) in enumerate(records):                                                # slot i stays frame i
        assert dst[dst_off[i]:dst_off[i + 1]] == (src[src_off[i]:src_off[i] + size] if st == 0 else b"")
    if with_dir:
        off, r = pm.read_directory(dst, n)
        assert off == dst_off and r == pm.Rec(0, len(dst) - D, len(dst), n, pm.NONE, pm.PATH_BATCH)


def test_model_rules(batch):
    src, src_off, records, _ = batch
    n = len(records)
    total = pm.pack(src, src_off, records, 1 << 30, True)[2].size
    # room: one byte short writes nothing and still says what was needed
    dst, dst_off, rec = pm.pack(src, src_off, records, total - 1, True)
    assert dst is None and rec.status == pm.ST_DSTSMALL and rec.size == total and dst_off[-1] == total
    assert pm.pack(src, src_off, records, total, True)[2].status == 0
    # records that lie: each an empty slot, the first of them reported
    lying = list(records)
    lying[1] = (0, src_off[2] - src_off[1] + 1)
    lying[5] = (0, 1 << 40)
    dst, dst_off, rec = pm.pack(src, src_off, lying, 1 << 30, False)
    assert rec.status == 0 and rec.first_bad_block == 1 and rec.n_blocks == n - 3
    assert dst_off[1] == dst_off[2] and dst_off[5] == dst_off[6]
    off2 = list(src_off)
    off2[-1] = len(src) + 1                                                                  # a span past srcBytes
    assert pm.pack(src, off2, records, 1 << 30, False)[2].first_bad_block == n - 1
    off3 = list(src_off)
    off3[2] = off3[1] - 1                                                                    # descending: frame 1 lies; frame 2's window only grows
    assert pm.pack(src, off3, records, 1 << 30, False)[2].first_bad_block == 1
    # a length the directory's u32 cannot say: a faked record, no buffer
    big = [(0, 1 << 32), (0, 5)]
    dst, dst_off, rec = pm.pack(None, [0, 1 << 33, (1 << 33) + 5], big, 1 << 40, True, src_bytes=1 << 34)
    assert dst is None and rec.status == pm.ST_SRCLARGE and rec.size == 32 + (1 << 32) + 5 and rec.first_bad_block == pm.NONE
    assert pm.pack(None, [0, 1 << 33, (1 << 33) + 5], big, 1 << 40, False, src_bytes=1 << 34)[2].status == 0
    assert pm.pack(None, [0, 1 << 33, (1 << 33) + 5], [(0, 0xFFFFFFFF), (0, 5)], 1 << 40, True, src_bytes=1 << 34)[2].status == 0


def test_model_refuses_forged_directories(batch):
    src, src_off, records, _ = batch
    n = len(records)
    dst, dst_off, _ = pm.pack(src, src_off, records, 1 << 30, True)
    D = pm.directory_size(n)

    def put32(b, at, v):
        return b[:at] + struct.pack("<I", v & 0xFFFFFFFF) + b[at + 4:]
    zeros = [0] * (n + 1)
    for forged, nn, st in ((put32(dst, 0, pm.DIR_MAGIC ^ 1), n, pm.ST_FRAMETYPE), (put32(dst, 8, pm.DIR_TAG ^ 0x100), n, pm.ST_FRAMETYPE),
                           (put32(dst, 12, n + 1), n, pm.ST_FRAMESIZE), (put32(dst, 12, n - 1), n, pm.ST_FRAMESIZE),
                           (dst, n + 1, pm.ST_FRAMESIZE), (dst, n - 1, pm.ST_FRAMESIZE),
                           (put32(dst, 24 + 4 * 2, struct.unpack_from("<I", dst, 32)[0] + 1), n, pm.ST_FRAMESIZE),
                           (put32(dst, 16, struct.unpack_from("<I", dst, 16)[0] + 1), n, pm.ST_FRAMESIZE),
                           (dst[:D - 1], n, pm.ST_INCOMPLETE), (dst[:-1], n, pm.ST_INCOMPLETE), (dst[:23], n, pm.ST_INCOMPLETE)):
        off, r = pm.read_directory(forged, nn)
        assert off == [0] * (nn + 1) and r == pm.Rec(st, 0, 0, 0, pm.NONE, pm.PATH_BATCH), (st, r)
    assert zeros == [0] * (n + 1)


def test_directory_size_agrees(L):
    for n in (0, 1, 1000):
        assert L.lz4f_mi355x_packDirectorySize(n) == pm.directory_size(n) == 24 + 4 * n


def test_peek_agrees_with_the_model(L, batch):
    src, src_off, records, _ = batch
    dst, _, _ = pm.pack(src, src_off, records, 1 << 30, True)
    head = dst[:24]

    def peek(b):
        n, fb = ctypes.c_uint32(77), ctypes.c_uint64(77)
        r = L.lz4f_mi355x_peekPackDirectory(b, len(b), ctypes.byref(n), ctypes.byref(fb))
        if L.LZ4F_isError(r):
            assert (n.value, fb.value) == (77, 77), "outputs written on an error"
            return (1 << 64) - r, 0, 0, 0
        return 0, r, n.value, fb.value
    assert peek(head) == pm.peek(head) == (0, pm.directory_size(len(records)), len(records), len(dst) - pm.directory_size(len(records)))
    assert peek(dst[:100]) == pm.peek(head)                                                  # more than the head is fine
    wrong_magic = struct.pack("<I", pm.DIR_MAGIC + 1) + head[4:]                             # (the trailer's skippable magic)
    wrong_tag = head[:8] + b"LZIX" + head[12:]
    wrong_payload = head[:4] + struct.pack("<I", 16 + 4 * len(records) + 4) + head[8:]
    for b, st in ((head[:23], pm.ST_INCOMPLETE), (b"", pm.ST_INCOMPLETE), (wrong_magic, pm.ST_FRAMETYPE), (wrong_tag, pm.ST_FRAMETYPE),
                  (wrong_payload, pm.ST_FRAMESIZE)):
        assert peek(b) == pm.peek(b) == (st, 0, 0, 0), st
    # NULL outputs are accepted; a NULL head is an incomplete one
    assert L.lz4f_mi355x_peekPackDirectory(head, 24, None, None) == pm.directory_size(len(records))
    assert (1 << 64) - L.lz4f_mi355x_peekPackDirectory(None, 24, None, None) == pm.ST_INCOMPLETE


def test_header_declares_library_exports_ffi_binds(L):
    hdr = open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()
    declared = set(re.findall(r"^LZ4F_MI355X_API[^;(]*?\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", hdr, flags=re.M))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in _ffi.DECLARED_SYMBOLS, s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is ctypes.c_size_t, s
    assert len(L.lz4f_mi355x_dev_packFrames.argtypes) == 11 and len(L.lz4f_mi355x_dev_readPackDirectory.argtypes) == 6
    assert re.search(r"#define\s+LZ4F_MI355X_PACK_DIRECTORY\s+0x1u", hdr)
    tile = int(re.search(r"#define\s+LZ4F_MI355X_PACK_TILE\s+(\d+)u", hdr).group(1))
    from lz4_frame_conduit_amd import device
    assert device.PACK_TILE == tile and tile % 16 == 0


def test_python_host_helpers(L, batch):
    from lz4_frame_conduit_amd import device
    src, src_off, records, _ = batch
    dst, _, _ = pm.pack(src, src_off, records, 1 << 30, True)
    assert device.pack_directory_size(1000) == 4024
    assert device.peek_pack_directory(dst[:24]) == pm.peek(dst[:24])[1:]
    with pytest.raises(device.DeviceCodecError, match="frameHeader_incomplete"):
        device.peek_pack_directory(dst[:23])
    with pytest.raises(ValueError):
        device.peek_pack_directory("a string")
    with pytest.raises(ValueError):
        device.pack_directory_size(-1)


def test_calls_without_engine_answer_generic(L):
    for r in (L.lz4f_mi355x_dev_packFrames(None, 0, None, 0, None, None, None, 0, None, 0, None),
              L.lz4f_mi355x_dev_packFrames(None, 3, None, 0, None, None, None, 0, None, 1, None),
              L.lz4f_mi355x_dev_readPackDirectory(None, 0, None, 0, None, None),
              L.lz4f_mi355x_dev_readPackDirectory(None, 3, None, 0, None, None)):
        assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
