"""What lz4f_mi355x_dev_splitFrames computes, restated in Python from include/lz4f_mi355x.h: the serial walk over a concatenated
stream - skippable frames stepped over, LZ4 frames listed, the first thing that is neither stops it - and what the call writes
for a given max_frames.  No payload is parsed and no checksum verified.  tests/test_split_model_cpu.py holds the walk to the oracle;
tests/test_gpu_split_frames.py holds the device to the walk.

The case builders are here too, shared by both tests.  A builder says what it planted (where every true frame starts, where the
walk stops and why) as it appends the bytes, so the expectation does not come from the model: the CPU test asserts that the two
agree."""
import struct
from collections import namedtuple

import numpy as np

import oracle

NONE = 0xFFFFFFFF
ST_MAXBLOCK, ST_VERSION, ST_RESERVED, ST_DSTSMALL, ST_INCOMPLETE, ST_FRAMETYPE, ST_HEADERCK = 2, 6, 8, 11, 12, 13, 17
FRAME_MAGIC, SKIP_MAGIC, LEGACY_MAGIC = 0x184D2204, 0x184D2A50, 0x184C2102
FLAG_SKIPPABLE = 0x100
PATH_BATCH, PATH_PARALLEL_WALK = 0x1000, 0x004
SPLIT_CHUNK = 16384                # the candidate pass's chunk (split_batch.cuh: SP_CHUNK)
SPLIT_SHARE = 256                  # LZ4F_MI355X_SPLIT_SHARE

Rec = namedtuple("Rec", "status size consumed n_blocks first_bad_block flags")     # flags: without the path bits
Walk = namedtuple("Walk", "starts pos status bytes skipped")

_M = 0xFFFFFFFF
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def le32(v): return struct.pack("<I", v & _M)
def u32(b, at=0): return struct.unpack_from("<I", b, at)[0]


def _rotl(x, r): return ((x << r) | (x >> (32 - r))) & _M


def xxh32_small(b: bytes) -> int:
    """XXH32, seed 0, of fewer than 16 bytes: all a header's descriptor ever is."""
    assert len(b) < 16
    h, i = (_P5 + len(b)) & _M, 0
    while i + 4 <= len(b):
        h = (_rotl((h + u32(b, i) * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < len(b):
        h = (_rotl((h + b[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15; h = (h * _P2) & _M; h ^= h >> 13; h = (h * _P3) & _M; h ^= h >> 16
    return h


# ---- the model ----
def step(S: bytes, pos: int):
    """What stands at S[pos:]: ("skip", bytes), ("frame", bytes) or ("stop", status)."""
    cap = len(S) - pos
    if cap < 7:
        return "stop", ST_INCOMPLETE
    magic = u32(S, pos)
    if magic & 0xFFFFFFF0 == SKIP_MAGIC:
        if cap < 8 or cap < 8 + u32(S, pos + 4):
            return "stop", ST_INCOMPLETE
        return "skip", 8 + u32(S, pos + 4)
    if magic != FRAME_MAGIC:
        return "stop", ST_FRAMETYPE
    flg, bd = S[pos + 4], S[pos + 5]
    if (flg >> 1) & 1:
        return "stop", ST_RESERVED
    if (flg >> 6) & 3 != 1:
        return "stop", ST_VERSION
    hsize = 7 + (8 if (flg >> 3) & 1 else 0) + (4 if flg & 1 else 0)
    if cap < hsize:
        return "stop", ST_INCOMPLETE
    if bd >> 7:
        return "stop", ST_RESERVED
    if (bd >> 4) & 7 < 4:
        return "stop", ST_MAXBLOCK
    if bd & 15:
        return "stop", ST_RESERVED
    if (xxh32_small(S[pos + 4:pos + hsize - 1]) >> 8) & 0xFF != S[pos + hsize - 1]:
        return "stop", ST_HEADERCK
    bs, bck = 1 << (8 + 2 * ((bd >> 4) & 7)), (flg >> 4) & 1
    at = hsize
    while True:
        if cap - at < 4:
            return "stop", ST_INCOMPLETE
        w = u32(S, pos + at)
        at += 4
        if w == 0:
            break
        csz = w & 0x7FFFFFFF
        if csz > bs:
            return "stop", ST_MAXBLOCK
        if cap - at < csz + 4 * bck:
            return "stop", ST_INCOMPLETE
        at += csz + 4 * bck
    tail = 4 if (flg >> 2) & 1 else 0
    if cap - at < tail:
        return "stop", ST_INCOMPLETE
    return "frame", at + tail


def walk(S: bytes) -> Walk:
    pos, starts, nbytes, skipped = 0, [], 0, False
    while pos < len(S):
        kind, v = step(S, pos)
        if kind == "stop":
            return Walk(starts, pos, v, nbytes, skipped)
        if kind == "skip":
            skipped = True
        else:
            starts.append(pos)
            nbytes += v
        pos += v
    return Walk(starts, pos, 0, nbytes, skipped)


def outputs(w: Walk, max_frames: int):
    """-> (the max_frames + 1 offsets, the record)"""
    n = len(w.starts)
    m = min(n, max_frames)
    fill = w.starts[max_frames] if n > max_frames else w.pos
    off = list(w.starts[:m]) + [fill] * (max_frames + 1 - m)
    status = w.status if w.status else (ST_DSTSMALL if n > max_frames else 0)
    return off, Rec(status, w.bytes, w.pos, n, n if w.status else NONE, FLAG_SKIPPABLE if w.skipped else 0)


def split(S: bytes, max_frames: int):
    return outputs(walk(S), max_frames)


def nodes(S: bytes) -> int:
    """The candidate pass's nodes: position 0, every LZ4 magic whose header parses, every skippable magic whose frame fits."""
    n, at = 1, S.find(b"\x4D\x18", 0)
    while at >= 0:
        p = at - 2
        if p > 0:
            magic = u32(S, p)
            if magic == FRAME_MAGIC or magic & 0xFFFFFFF0 == SKIP_MAGIC:
                kind, v = step(S, p)
                head_ok = kind != "stop" or (magic == FRAME_MAGIC and _head_parses(S, p))
                n += 1 if head_ok else 0
        at = S.find(b"\x4D\x18", at + 1)
    return n


def _head_parses(S: bytes, p: int) -> bool:
    """An LZ4 magic at p: does its header parse in the bytes that remain?  (A frame that is cut behind its header is a node too.)"""
    cap = len(S) - p
    if cap < 7:
        return False
    flg = S[p + 4]
    hsize = 7 + (8 if (flg >> 3) & 1 else 0) + (4 if flg & 1 else 0)
    if cap < hsize:
        return False
    return step(S[p:p + hsize] + b"\0\0\0\0" * 2, 0)[0] == "frame"        # the header alone, an EndMark and a checksum word behind it


def node_cap(max_frames: int, src_bytes: int) -> int:
    return min(max_frames + src_bytes // SPLIT_SHARE + 64, 0xFFFFFFF0)


# ---- frames by hand ----
def head(bsid=4, indep=1, bck=0, cck=0, csize=None, dictid=None) -> bytes:
    flg = (1 << 6) | (indep << 5) | (bck << 4) | ((csize is not None) << 3) | (cck << 2) | (dictid is not None)
    d = bytes([flg, bsid << 4]) + (struct.pack("<Q", csize) if csize is not None else b"") + (le32(dictid) if dictid is not None else b"")
    return le32(FRAME_MAGIC) + d + bytes([(xxh32_small(d) >> 8) & 0xFF])


def stored_frame(payloads, **h) -> bytes:
    """A frame of stored blocks, its checksums true (so that every decoder takes it)."""
    out = bytearray(head(**h))
    for p in payloads:
        out += le32(0x80000000 | len(p)) + p
        if h.get("bck"):
            out += le32(oracle.xxh32(p))
    out += le32(0)
    if h.get("cck"):
        out += le32(oracle.xxh32(b"".join(payloads)))
    return bytes(out)


def skippable(payload: bytes, k: int = 0) -> bytes:
    return le32(SKIP_MAGIC | k) + le32(len(payload)) + payload


def noise(name: str, n: int) -> bytes:
    """Seeded bytes without 0x18: no magic in them, whatever stands around them."""
    a = np.random.default_rng(list(name.encode())).integers(0, 255, n, dtype=np.uint8)
    a[a >= 0x18] += 1
    return a.tobytes()


class Stream:
    """A stream under construction, and what was planted in it."""
    def __init__(self):
        self.buf, self.starts, self.bytes, self.skipped, self.status, self.pos = bytearray(), [], 0, False, 0, None

    def frame(self, f: bytes):
        assert self.pos is None
        self.starts.append(len(self.buf)); self.buf += f; self.bytes += len(f)
        return self

    def skip(self, f: bytes):
        assert self.pos is None
        self.buf += f; self.skipped = True
        return self

    def stop(self, tail: bytes, status: int):
        """`tail` is where the walk stops, with `status`"""
        assert self.pos is None and status
        self.pos, self.status = len(self.buf), status
        self.buf += tail
        return self

    def pad_to(self, target: int, name: str):
        """a frame of one stored block, so long that the next thing starts at `target`"""
        n = target - len(self.buf) - 15
        assert 0 <= n <= 65536, (target, len(self.buf))
        return self.frame(stored_frame([noise(name, n)]))

    def planted(self) -> Walk:
        return Walk(self.starts, len(self.buf) if self.pos is None else self.pos, self.status, self.bytes, self.skipped)

    def data(self) -> bytes:
        return bytes(self.buf)


Case = namedtuple("Case", "name stream planted max_frames serial")     # max_frames None: the frames there are; serial: the list overflows


def _case(name, s: Stream, max_frames=None, serial=False) -> Case:
    return Case(name, s.data(), s.planted(), max_frames, serial)


def oracle_frames():
    """(prefs as words, frame, input): oracle.conduit_compress under varied prefs"""
    text = (b"the quick brown fox jumps over the lazy dog; " * 40 + bytes(range(256))) * 200
    out = []
    for k, (bsid, indep, cck, bck, csize, n) in enumerate([(4, 1, 0, 0, 0, 70000), (4, 0, 1, 0, 0, 200000), (5, 1, 0, 1, 1, 300000), (6, 0, 1, 1, 0, 150000),
                                                            (7, 1, 0, 0, 0, 1000), (0, 0, 0, 0, 0, 0), (4, 1, 1, 1, 1, 13), (5, 0, 0, 0, 1, 65536)]):
        x = (noise("orc%d" % k, n // 3) + text)[:n] if n else b""
        assert len(x) == n
        p = oracle.mkprefs(bsid=bsid, indep=indep, cck=cck, bck=bck, csize=n if csize else 0, dictid=0x1234 if k == 3 else 0)
        out.append(((bsid, indep, cck, bck, csize), oracle.conduit_compress(x, p), x))
    return out


def grammar_stream() -> Stream:
    s = Stream()
    for k, h in enumerate([dict(), dict(dictid=7), dict(csize=5), dict(csize=5, dictid=0xFFFFFFFF)]):      # headers of 7, 11, 15, 19 bytes
        s.frame(stored_frame([noise("g%d" % k, 5)], **h))
    s.frame(stored_frame([noise("bck", 100), noise("bck2", 1)], bck=1))
    s.frame(stored_frame([noise("cck", 33)], cck=1))
    s.frame(stored_frame([noise("both", 17), b"", noise("both2", 300)], bck=1, cck=1, csize=317))           # an empty stored block: 0x80000000
    s.frame(stored_frame([b""]))
    for bsid in (4, 5, 6, 7):
        for indep in (0, 1):
            s.frame(stored_frame([noise("bs%d%d" % (bsid, indep), 1 << (6 + bsid))], bsid=bsid, indep=indep))
    for _, f, _ in oracle_frames():
        s.frame(f)
    for _ in range(70):
        s.frame(stored_frame([]))                                                                            # 11 bytes: header + EndMark
    for k in range(70):
        s.frame(stored_frame([], cck=1) if k % 2 else stored_frame([], dictid=k))                            # 15 bytes, both ways
    return s


def position_streams():
    """Frames whose magic or header straddles a 16-byte load unit, and the candidate pass's chunk boundary"""
    out = []
    s = Stream()
    for k, r in enumerate((13, 14, 15, 16)):                                  # a magic's four splits across a 16-byte unit
        s.pad_to(64 * (k + 1) + r, "u%d" % k)
        s.frame(stored_frame([noise("uf%d" % k, 3)], csize=3, dictid=9))
    out.append(_case("pos/unit", s))
    for r in (-3, -2, -1, 0):                                                 # ... across the chunk boundary
        s = Stream()
        s.pad_to(SPLIT_CHUNK + r, "c%d" % r)
        s.frame(stored_frame([noise("cf%d" % r, 40)], bck=1))
        s.frame(stored_frame([]))
        out.append(_case("pos/chunk%+d" % r, s))
    for r in (-18, -10, -6, -5):                                              # a 19-byte header across it: the cut in every field
        s = Stream()
        s.pad_to(SPLIT_CHUNK + r, "h%d" % r)
        s.frame(stored_frame([noise("hf%d" % r, 9)], csize=9, dictid=1, cck=1))
        out.append(_case("pos/header%+d" % r, s))
    return out


def skippable_streams():
    out = []
    s = Stream()
    s.frame(stored_frame([noise("s0", 20)]))
    for k in range(16):                                                       # each of the 16 magics, between frames
        s.skip(skippable(noise("sk%d" % k, k), k))
        s.frame(stored_frame([noise("sf%d" % k, k + 1)]))
    s.skip(skippable(b"", 3)).skip(skippable(noise("end", 100), 15))          # size 0; at the end
    out.append(_case("skip/magics", s))
    from lz4_frame_conduit_amd import conduit                               # this library's in-band trailer: a skippable frame behind the frame
    s = Stream()
    for _, f, _ in oracle_frames()[:3]:
        listed = conduit.appendBlockList(f)
        assert listed[:len(f)] == f and len(listed) > len(f) + 8
        s.frame(f).skip(listed[len(f):])
    s.frame(stored_frame([noise("behind the trailer", 9)]))
    out.append(_case("skip/trailer", s))
    inner = stored_frame([noise("inner", 50)], cck=1)
    s = Stream()
    s.skip(skippable(b"ab", 0)).frame(stored_frame([noise("a", 9)])).skip(skippable(inner, 7)).frame(stored_frame([noise("b", 9)])).skip(skippable(inner + inner, 1))
    out.append(_case("skip/holds_a_frame", s))
    return out


def nested(level: int, name: str) -> bytes:
    f = stored_frame([noise(name, 60)], cck=1)
    for k in range(level):
        f = stored_frame([noise("%s/%d" % (name, k), 7 + k) + f + noise("%s/%d'" % (name, k), 5)])
    return f


def false_streams():
    out = []
    inner = stored_frame([noise("in", 90), noise("in2", 10)], bck=1, cck=1)
    s = Stream()
    s.frame(stored_frame([inner + noise("f0", 30)]))                          # at payload offset 0
    s.frame(stored_frame([b"\x01" + inner + noise("f1", 30)]))               # at 1
    s.frame(stored_frame([noise("f2", 30) + inner], bck=1))                   # at the payload's end
    s.frame(stored_frame([noise("f3", 30), inner, noise("f3'", 1)]))          # a whole block
    out.append(_case("false/whole_frame", s))
    # an inner frame that lacks only its EndMark, at the very end of the last block: the outer EndMark closes it too
    open_inner = stored_frame([noise("open", 40)])[:-4]
    s = Stream()
    s.frame(stored_frame([noise("o0", 12)]))
    s.frame(stored_frame([noise("o1", 25), noise("o2", 3) + open_inner]))
    s.frame(stored_frame([noise("o3", 12)]))
    assert step(s.data(), s.starts[1] + 7 + 4 + 25 + 4 + 3) == ("frame", len(open_inner) + 4)               # the false node ends on the next frame's start
    out.append(_case("false/closed_by_outer_endmark", s))
    s = Stream()
    s.frame(nested(3, "n0")).frame(nested(1, "n1")).frame(nested(3, "n2"))
    out.append(_case("false/nested", s))
    s = Stream()
    h = head(cck=1)
    bad_ck = h[:6] + bytes([h[6] ^ 0x40])
    reserved = le32(FRAME_MAGIC) + bytes([0x62, 0x40, 0])
    s.frame(stored_frame([le32(FRAME_MAGIC), noise("m", 5) + le32(FRAME_MAGIC) * 3, bad_ck + noise("m2", 20), reserved + noise("m3", 20), le32(SKIP_MAGIC | 4) + le32(1 << 20),
                          noise("m4", 13) + le32(LEGACY_MAGIC) + le32(FRAME_MAGIC)[:3]]))
    s.frame(stored_frame([h]))                                                # a header alone, in the last bytes of a payload: a node that does not end
    s.frame(stored_frame([noise("m5", 4)]))
    out.append(_case("false/magics", s))
    return out


def five(k_bad=None) -> Stream:
    s = Stream()
    for k in range(5):
        f = stored_frame([noise("five%d" % k, 100 + k), noise("five%d'" % k, 7)], bsid=4, cck=k % 2)
        if k == k_bad:
            at = 7 + 4 + 100 + k
            s.stop(f[:at] + le32(65537) + f[at + 4:] + stored_frame([]), ST_MAXBLOCK)          # a size word above the block size
            break
        s.frame(f)
    return s


def stop_streams():
    out = []
    s = five()
    s.stop(noise("junk", 64), ST_FRAMETYPE)                                                    # random bytes behind the last frame
    out.append(_case("stop/junk", s))
    s = five()
    s.stop(le32(LEGACY_MAGIC) + le32(5) + b"abcde", ST_FRAMETYPE)
    out.append(_case("stop/legacy", s))
    for k in (0, 3):
        out.append(_case("stop/word_above_block_size/%d" % k, five(k)))
    for n in (1, 2, 3):                                                                        # a frame that ends 1..3 bytes before srcBytes
        s = five()
        s.stop(le32(FRAME_MAGIC)[:n], ST_INCOMPLETE)
        out.append(_case("stop/%d_bytes_behind" % n, s))
    h = head()
    for name, tail, st in (("reserved_flg", le32(FRAME_MAGIC) + bytes([0x62, 0x40, 0]) + le32(0), ST_RESERVED),
                           ("version", le32(FRAME_MAGIC) + bytes([0x20, 0x40, 0]) + le32(0), ST_VERSION),
                           ("reserved_bd", le32(FRAME_MAGIC) + bytes([0x60, 0x41, 0]) + le32(0), ST_RESERVED),
                           ("block_size_id", le32(FRAME_MAGIC) + bytes([0x60, 0x30, 0]) + le32(0), ST_MAXBLOCK),
                           ("header_checksum", h[:6] + bytes([h[6] ^ 1]) + le32(0), ST_HEADERCK),
                           ("skippable_cut", skippable(noise("cut", 30))[:-1], ST_INCOMPLETE)):
        s = five()
        s.stop(tail, st)
        out.append(_case("stop/" + name, s))
    s = Stream()
    s.stop(noise("root", 100), ST_FRAMETYPE)                                                   # nothing at all: the root is no frame
    out.append(_case("stop/at_once", s))
    return out


def truncation_stream():
    """Two frames; the GPU test cuts the second at every byte -> (stream, the first frame's length)"""
    a = stored_frame([noise("ta", 6)], cck=1)
    b = stored_frame([noise("tb", 3), b"", noise("tb2", 2)], bck=1, cck=1, csize=5, dictid=2)
    return a + b, len(a)


def max_frames_cases():
    s = Stream()
    s.skip(skippable(noise("front", 40), 13))
    for k in range(6):
        s.frame(stored_frame([noise("mf%d" % k, 30 + k)]))
        if k % 2:
            s.skip(skippable(b"xy", k))
    return [_case("max_frames/%s" % name, s, m) for name, m in (("n", 6), ("n-1", 5), ("1", 1), ("4n", 24))]


def depth_cases():
    e = stored_frame([])
    out = []
    for n in (2051, 66000):                                                    # the scan carries across tiles; a chain longer than 2^16
        s = Stream()
        s.buf, s.starts, s.bytes = bytearray(e * n), list(range(0, 11 * n, 11)), 11 * n
        out.append(_case("depth/%d" % n, s))
    s = Stream()
    s.frame(stored_frame([b"\x07"] * 5000))                                    # the long walk of one node
    s.frame(stored_frame([b"\x08"]))
    out.append(_case("depth/5000_blocks", s))
    return out


def overflow_case() -> Case:
    """One stored block filled with valid 7-byte headers: more nodes than the list holds for this srcBytes and max_frames"""
    s = Stream()
    s.frame(stored_frame([head() * (65536 // 7)]))
    s.frame(stored_frame([noise("ov", 10)]))
    return _case("overflow", s, 2, True)


def short_stream() -> Stream:
    s = Stream()
    s.skip(skippable(b"front", 2))
    for k in range(4):
        s.frame(stored_frame([noise("sh%d" % k, 21 + 5 * k)], cck=k % 2, bck=k // 2))
    s.skip(skippable(b"", 0))
    return s


def all_cases():
    """Every case that is one stream and one call (the GPU test adds shifts, cuts, chains and the run-twice)."""
    return ([_case("grammar", grammar_stream()), _case("short", short_stream())] + position_streams() + skippable_streams() + false_streams() + stop_streams() +
            max_frames_cases() + depth_cases() + [overflow_case()])
