"""What lz4f_mi355x_dev_packFrames and lz4f_mi355x_dev_readPackDirectory compute, restated in Python from include/lz4f_mi355x.h:
the lengths from the records and their windows, the offsets, the packed bytes, the frame directory and the two records.  The GPU
tests hold every result to this; tests/test_pack_model_cpu.py holds this to the oracle and to the library's host helpers."""
import struct
from collections import namedtuple

NONE = 0xFFFFFFFF
PATH_BATCH = 0x1000
ST_SRCLARGE, ST_DSTSMALL, ST_INCOMPLETE, ST_FRAMETYPE, ST_FRAMESIZE = 10, 11, 12, 13, 14
DIR_MAGIC, DIR_TAG, DIR_HEAD = 0x184D2A5D, 0x44505A4C, 24
DIR_MOST_FRAMES = (0xFFFFFFFF - 16) // 4

Rec = namedtuple("Rec", "status size consumed n_blocks first_bad_block flags")


def directory_size(n: int) -> int:
    return DIR_HEAD + 4 * n


def lengths(src_off, records, src_bytes):
    """records: (status, size) per frame -> (L, the first record with status 0 that lies, or NONE)."""
    L, first_bad = [], NONE
    for i, (status, size) in enumerate(records):
        s0, s1 = src_off[i], src_off[i + 1]
        if status != 0:
            L.append(0)
            continue
        ok = s0 <= s1 <= src_bytes and size <= s1 - s0
        if not ok and first_bad == NONE:
            first_bad = i
        L.append(size if ok else 0)
    return L, first_bad


def directory(L) -> bytes:
    n = len(L)
    return struct.pack("<IIIIQ", DIR_MAGIC, 16 + 4 * n, DIR_TAG, n, sum(L)) + struct.pack("<%dI" % n, *L)


def pack(src, src_off, records, dst_bytes, directory_flag, src_bytes=None):
    """-> (dst bytes or None, dst_off, Rec).  src: bytes (None: lengths only, with src_bytes given - no byte is copied then);
    dst: the d_dst_off[n] bytes the call writes, None when it writes none."""
    n = len(records)
    assert len(src_off) == n + 1
    if src_bytes is None:
        src_bytes = len(src)
    L, first_bad = lengths(src_off, records, src_bytes)
    D = directory_size(n) if directory_flag else 0
    dst_off = [D]
    for x in L:
        dst_off.append(dst_off[-1] + x)
    status = 0
    if directory_flag and (any(x > 0xFFFFFFFF for x in L) or n > DIR_MOST_FRAMES):
        status = ST_SRCLARGE
    if dst_off[-1] > dst_bytes:
        status = ST_DSTSMALL
    rec = Rec(status, dst_off[-1], sum(L), sum(1 for x in L if x), first_bad, PATH_BATCH)
    if status or src is None:
        return None, dst_off, rec
    out = bytearray(directory(L) if directory_flag else b"")
    for i, x in enumerate(L):
        out += bytes(src[src_off[i]:src_off[i] + x])
    assert len(out) == dst_off[-1]
    return bytes(out), dst_off, rec


def peek(head: bytes):
    """The fixed part -> (status, directory bytes, n_frames, frames bytes)."""
    if len(head) < DIR_HEAD:
        return ST_INCOMPLETE, 0, 0, 0
    magic, payload, tag, n, fb = struct.unpack_from("<IIIIQ", head)
    if magic != DIR_MAGIC or tag != DIR_TAG:
        return ST_FRAMETYPE, 0, 0, 0
    if n > DIR_MOST_FRAMES or payload != 16 + 4 * n:
        return ST_FRAMESIZE, 0, 0, 0
    return 0, directory_size(n), n, fb


def read_directory(pack_bytes_: bytes, n: int):
    """The stream (all the bytes the receiver has) and the n_frames it expects -> (src_off, Rec)."""
    refuse = lambda st: ([0] * (n + 1), Rec(st, 0, 0, 0, NONE, PATH_BATCH))
    have = len(pack_bytes_)
    st, D, stored, fb = peek(pack_bytes_[:DIR_HEAD])
    if st:
        return refuse(st)
    if stored != n:
        return refuse(ST_FRAMESIZE)
    if have < D:
        return refuse(ST_INCOMPLETE)
    L = struct.unpack_from("<%dI" % n, pack_bytes_, DIR_HEAD)
    if sum(L) != fb:
        return refuse(ST_FRAMESIZE)
    if D + fb > have:
        return refuse(ST_INCOMPLETE)
    off = [D]
    for x in L:
        off.append(off[-1] + x)
    return off, Rec(0, fb, D + fb, n, NONE, PATH_BATCH)
