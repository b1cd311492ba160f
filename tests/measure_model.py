"""A pure-Python model of lz4f_mi355x_dev_measureFrames' contract (test helper, not a test module).

measure(span) -> Measured(status, size, consumed, n_blocks, first_bad_block, flags & 0x1FF, W) for the first frame of a span:
the frame walk (header, size words, EndMark, the content checksum's word), then a token walk per block under the block
grammar's rules that need neither output bytes nor history (tests/lz4_grammar.py's docstring, room = maxBlockSize).  Match
offsets, block checksums and content checksums are not looked at.  One verdict is the batch decoder's and not the format's: a span
with more blocks than a fifth of its bytes and two (empty stored blocks, 4 bytes each) is dstMaxSize_tooSmall to that decoder in any
window, so it is here (empty_stored_frame makes one; the oracle takes it).  W models the batch decoder's placement: the smallest window
in which every block has its provisional place (block b at b * maxBlockSize) and the room it decodes to (decoder_accepts).

The frame layout and the token grammar are restated here on purpose: nothing of the library under test is used.  frames() is
the corpus the measure tests share; oracle_verdict() what the oracle says about one of them (cached)."""
from __future__ import annotations

import collections
import functools
import glob
import os
import struct

NONE = 0xFFFFFFFF
MAGIC, SKIP0 = 0x184D2204, 0x184D2A50
(OK, GENERIC, MAXBLOCK, VERSION, BLOCKCK, RESERVED, INCOMPLETE, FRAMETYPE, FRAMESIZE, SRCPTR, HEADERCK, CONTENTCK) = (0, 1, 2, 6, 7, 8, 12, 13, 14, 15, 17, 18)
DSTSMALL = 11

Measured = collections.namedtuple("Measured", "status size consumed n_blocks first_bad flags W")

_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _xxh32_small(b: bytes) -> int:
    """XXH32, seed 0, of fewer than 16 bytes (a frame descriptor)."""
    assert len(b) < 16
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & _M
    h, i = (_P5 + len(b)) & _M, 0
    while i + 4 <= len(b):
        h = (rotl((h + int.from_bytes(b[i:i + 4], "little") * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < len(b):
        h = (rotl((h + b[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15; h = (h * _P2) & _M; h ^= h >> 13; h = (h * _P3) & _M; h ^= h >> 16
    return h


def block_size(p: bytes, room: int) -> int:
    """What a compressed block's payload decodes to, from its tokens alone; -1: malformed."""
    n = len(p)
    if n == 0:
        return -1
    ip = op = 0
    while True:
        if ip >= n:
            return -1
        tok = p[ip]; ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    return -1
                s = p[ip]; ip += 1; lit += s
                if s != 255:
                    break
        in_left, out_left = n - ip, room - op
        if lit + 12 > out_left or lit + 8 > in_left:          # must be the last sequence
            if lit != in_left or lit > out_left:
                return -1
            return op + lit
        ip += lit + 2; op += lit                              # (the two offset bytes: stepped over)
        ml = tok & 15
        if ml == 15:
            while True:
                if ip >= n:
                    return -1
                s = p[ip]; ip += 1; ml += s
                if ip + 4 >= n:
                    return -1
                if s != 255:
                    break
        ml += 4
        if ml + 5 > room - op:
            return -1
        op += ml


def walk(span: bytes):
    """The frame walk -> (status, flags, consumed, bs, [(size word, payload position)]); blocks only with status 0."""
    n = len(span)
    if n < 7:
        return INCOMPLETE, 0, 0, 0, []
    magic = int.from_bytes(span[:4], "little")
    if magic & 0xFFFFFFF0 == SKIP0:
        if n < 8 or n < 8 + int.from_bytes(span[4:8], "little"):
            return INCOMPLETE, 0, 0, 0, []
        return OK, 0x100, 8 + int.from_bytes(span[4:8], "little"), 0, []
    if magic != MAGIC:
        return FRAMETYPE, 0, 0, 0, []
    flg = span[4]
    if flg & 2:
        return RESERVED, 0, 0, 0, []
    if flg >> 6 != 1:
        return VERSION, 0, 0, 0, []
    hs = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if n < hs:
        return INCOMPLETE, 0, 0, 0, []
    bd = span[5]
    if bd & 0x80:
        return RESERVED, 0, 0, 0, []
    if (bd >> 4) & 7 < 4:
        return MAXBLOCK, 0, 0, 0, []
    if bd & 15:
        return RESERVED, 0, 0, 0, []
    if (_xxh32_small(span[4:hs - 1]) >> 8) & 0xFF != span[hs - 1]:
        return HEADERCK, 0, 0, 0, []
    bs, bck = 1 << (8 + 2 * ((bd >> 4) & 7)), 4 if flg & 0x10 else 0
    pos, blocks = hs, []
    while True:
        if n - pos < 4:
            return INCOMPLETE, flg, 0, bs, []
        w = int.from_bytes(span[pos:pos + 4], "little"); pos += 4
        if w == 0:
            break
        csz = w & 0x7FFFFFFF
        if csz > bs:
            return MAXBLOCK, flg, 0, bs, []
        if n - pos < csz + bck:
            return INCOMPLETE, flg, 0, bs, []
        if len(blocks) >= min(n // 5 + 2, 0x7FFFFFFF):         # the batch decoder's bound on a span's blocks, whatever the window
            return DSTSMALL, flg, 0, bs, []
        blocks.append((w, pos))
        pos += csz + bck
    if flg & 4:
        if n - pos < 4:
            return INCOMPLETE, flg, 0, bs, []
        pos += 4
    return OK, flg, pos, bs, blocks


def decoder_accepts(gots, bs: int, linked: bool, win: int) -> bool:
    """The batch decoder's placement (decode_batch.cuh) for blocks that decode to gots[b] bytes, in a window of win bytes: every
    block's provisional place b * bs lies inside the window; a block is decoded at its place (independent) or behind its
    predecessors (linked) into what is left of the window, at most bs, and must fit; a block with less than bs of room is judged
    by the block grammar against that room - unless it is the last one and win % bs != 0, when it is judged against bs as it
    should be.  So anything but that tight last block needs a whole block of room to be judged as measure judges it."""
    out = 0
    for b, g in enumerate(gots):
        if b * bs >= win:
            return False
        at = out if linked else b * bs
        room = min(win - at, bs)
        if g > room:
            return False
        if room < bs and not (b + 1 == len(gots) and win % bs != 0):
            return False
        out += g
    return True


def window(gots, bs: int, linked: bool) -> int:
    """The smallest window decoder_accepts takes."""
    if not gots:
        return 0
    w = out = 0
    for b, g in enumerate(gots):                              # what the rules that only ask for more ask for: a place, and room behind it
        w = max(w, b * bs + 1, (out if linked else b * bs) + g)
        out += g
    while not decoder_accepts(gots, bs, linked, w):           # (the others: a few steps at most)
        w += 1
    return w


def measure(span: bytes) -> Measured:
    st, flg, consumed, bs, blocks = walk(span)
    if st:
        return Measured(st, 0, 0, 0, NONE, flg & 0x1FF, 0)
    gots = []
    for b, (w, pos) in enumerate(blocks):
        csz = w & 0x7FFFFFFF
        g = csz if w >> 31 else block_size(span[pos:pos + csz], bs)
        if g < 0:
            return Measured(GENERIC, 0, consumed, len(blocks), b, flg & 0x1FF, 0)
        gots.append(g)
    size = sum(gots)
    if flg & 8 and not flg & 0x100 and int.from_bytes(span[6:14], "little") != size:
        return Measured(FRAMESIZE, size, consumed, len(blocks), NONE, flg & 0x1FF, 0)
    return Measured(OK, size, consumed, len(blocks), NONE, flg & 0x1FF, window(gots, bs, not flg & 0x20))


# ---- the frames the measure tests share ----
def skippable(payload: bytes, k: int = 0) -> bytes:
    return (SKIP0 + k).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload


FLUSH_BYTES = 33000                # the autoFlush frames: 5000-byte slices of this much -> 7 short blocks, whatever the block size


def empty_stored_frame(n: int, bsid: int = 4, linked: bool = False) -> bytes:
    """A frame of n empty stored blocks (size word 0x80000000, 4 bytes each): valid to the oracle, decoding to nothing."""
    flg = (1 << 6) | ((0 if linked else 1) << 5)
    h = bytes([flg, bsid << 4])
    return struct.pack("<I", MAGIC) + h + bytes([(_xxh32_small(h) >> 8) & 0xFF]) + struct.pack("<I", 0x80000000) * n + bytes(4)


@functools.lru_cache(maxsize=None)
def made_frames():
    """Oracle-made frames: bsid 4-7 x linked / independent x {plain, block checksums, content checksum + content size, dictID +
    autoFlush in 5000-byte slices}; empty frames; spans that start with a skippable frame."""
    import oracle
    from lz4_frame_conduit_amd import datagen
    s50 = datagen.synth50(5 << 20, 77).tobytes()
    txt = datagen.synth_text(300 << 10, 5).tobytes()
    out = []
    for bsid in (4, 5, 6, 7):
        bs = 1 << (8 + 2 * bsid)
        for indep in (0, 1):
            for k, (bck, cck, csize, dictid, af) in enumerate([(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 1, 0, 0), (1, 1, 0, 7, 1)]):
                if af:
                    data = txt[1000 * bsid:1000 * bsid + FLUSH_BYTES]
                elif bsid == 4:
                    data = txt[:2 * bs + 1234 + 100 * k]
                else:
                    data = s50[k * 512:k * 512 + bs + (bs >> 3) + 77 * k]
                p = oracle.mkprefs(bsid=bsid, indep=indep, bck=bck, cck=cck, csize=len(data) if csize else 0, dictid=dictid, autoflush=af)
                out.append(("made/b%d/i%d/k%d" % (bsid, indep, k), oracle.conduit_compress(data, p, slice_=5000 if af else 16384)))
        out.append(("made/empty/b%d" % bsid, oracle.conduit_compress(b"", oracle.mkprefs(bsid=bsid, cck=bsid & 1, csize=0))))
    out.append(("made/skippable_first", skippable(b"not a frame" * 7) + out[3][1]))
    out.append(("made/skippable_first_k9", skippable(b"x", 9) + out[0][1]))
    out.append(("made/empty_skippable", skippable(b"")))
    return out


@functools.lru_cache(maxsize=None)
def frames():
    """[(name, frame bytes)]: the block grammar's corpus, the frame grammar's, the golden files, the made frames."""
    import frame_edges
    import lz4_grammar
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    fs = [("grammar/" + n, f) for n, f, _ in lz4_grammar.corpus()]
    fs += [("edges/" + n, f) for n, f, _ in frame_edges.corpus()]
    fs += [("golden/" + os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(golden, "*.lz4")))]
    fs += list(made_frames())
    assert len({n for n, _ in fs}) == len(fs)
    return fs


@functools.lru_cache(maxsize=None)
def model_of(frame: bytes) -> Measured:
    return measure(frame)


def ample(frame: bytes) -> int:
    """A window in which the oracle and the decoders judge every block of the frame by its own defects: a whole block for every
    size word that may be one (a lenient count), and one more."""
    if len(frame) < 7 or int.from_bytes(frame[:4], "little") != MAGIC:
        return 1 << 16
    flg, bsid = frame[4], (frame[5] >> 4) & 7
    pos, n, bck = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0), 0, 4 if flg & 0x10 else 0
    while pos + 4 <= len(frame):
        w = int.from_bytes(frame[pos:pos + 4], "little")
        if w == 0:
            break
        pos += 4 + (w & 0x7FFFFFFF) + bck
        n += 1
    return (n + 1) << (8 + 2 * max(bsid, 4))


@functools.lru_cache(maxsize=None)
def oracle_verdict(frame: bytes):
    """(error name or None, output bytes or None, consumed) by the oracle, in an ample window."""
    import oracle
    try:
        out, used = oracle.decompress_frame(frame, cap=ample(frame))
        return None, out, used
    except oracle.OracleError as e:
        return str(e), None, 0


# ---- a frame with every match offset made valid (the tests' proof that an oracle-only rejection is about offsets) ----
def _offset_places(p: bytes, room: int):
    """[(position of the offset's two bytes in the payload, output position of the match)] of a payload block_size accepts."""
    n, ip, op, out = len(p), 0, 0, []
    while True:
        tok = p[ip]; ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                s = p[ip]; ip += 1; lit += s
                if s != 255:
                    break
        if lit + 12 > room - op or lit + 8 > n - ip:
            return out
        ip += lit; op += lit
        out.append((ip, op))
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                s = p[ip]; ip += 1; ml += s
                if s != 255:
                    break
        op += ml + 4


def with_valid_offsets(frame: bytes):
    """The frame (one that measure accepts) with every match offset set to 1 and its block checksums made right again; the content
    checksum is left as it is.  -> (frame, [(payload, bytes it decodes to)] of its compressed blocks, matches that no offset
    makes valid: those at a block's very start with no history in front, where 0 < offset <= op + hist has no solution)."""
    import oracle
    st, flg, consumed, bs, blocks = walk(frame)
    assert st == OK
    f, done, linked, payloads, hopeless = bytearray(frame), 0, not flg & 0x20, [], 0
    for w, pos in blocks:
        csz = w & 0x7FFFFFFF
        if w >> 31:
            done += csz
            continue
        for at, op in _offset_places(bytes(f[pos:pos + csz]), bs):
            f[pos + at:pos + at + 2] = b"\x01\x00"
            if op + (min(done, 65536) if linked else 0) < 1:
                hopeless += 1
        payload = bytes(f[pos:pos + csz])
        if flg & 0x10:
            f[pos + csz:pos + csz + 4] = struct.pack("<I", oracle.xxh32(payload))
        payloads.append((payload, block_size(payload, bs)))
        done += payloads[-1][1]
    return bytes(f), payloads, hopeless
