"""Frames with TWO flaws, and the written order that says which one decides (test helper, not a test module).

The other hostile corpora (lz4_grammar, frame_edges, dict_cases.planted, the forged indexes) put one flaw in a frame, so the code
that picks among failures - the atomicMin / ballot / `ck <= bad` merges that rebuild a sequential decoder's answer from parallel
work - only ever sees one.  Here every pair comes with its two flaws alone, so that a test can say "the pair's verdict is the
first flaw's", and the pairs are chosen so that the two flaws mostly have different error names.

Frames: block size ID 4, block checksums, content checksum (a content size only where `csize` needs the field); every shape as an
independent and as a linked frame; rebuilt identically from the case name (lz4_grammar's seeding).
  shapes       short5            five blocks of four sequences (linked: the first match reaches into the block in front)
               full3s / full3d   three full 64 KiB blocks of lz4_grammar's sparse / dense filler
               edge64/65/130     64, 65, 130 short blocks: flaws on both sides of the 64-entry groups the finishing kernels work in
  block atoms  cut          the payload ends inside a literal run (lit/cut/short_by_one's tail behind ordinary sequences)
               over         the block decodes to maxBlockSize + 1
               bck          one flipped bit in the block's checksum word
               word         a compressed block's size word says maxBlockSize + 1
               stored_over  a stored block of maxBlockSize + 1 bytes
  frame atoms  trunc.pay@b / trunc.bck@b / trunc.word@b   the span ends inside block b's payload / checksum word / size word
               trunc.end / trunc.cck                      ... before the EndMark / inside the content checksum's word
               room@b       the window ends inside block b's output (a window, not a byte of the frame: Case.room)
               csize        the header's content size is one too many (header checksum made right again)
               cck          one flipped bit in the content checksum
A name is shape/mode/flaw+flaw, the flaws in the order liblz4 meets them; shape/mode/clean is the frame without a flaw.

one_shot_verdict() is the paragraph "WHICH FLAW DECIDES" of include/lz4f_mi355x.h written out in Python, and nothing else:
the tests hold every one-shot call to it.  The drop-in surfaces have no order of their own: theirs is liblz4's, recorded in
tests/golden/flaw_pairs.json by tools/mint_flaw_pairs.py."""
from __future__ import annotations

import collections
import ctypes
import functools
import hashlib
import json
import os
import struct
import zlib

import oracle
from lz4_grammar import Frame, _fill, _rng

BSID, BS = 4, 65536
NONE = 0xFFFFFFFF
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flaw_pairs.json")
MODES = ("indep", "linked")
SHAPES = {"short5": (5, "short"), "full3s": (3, "sparse"), "full3d": (3, "dense"), "edge64": (64, "short"), "edge65": (65, "short"),
          "edge130": (130, "short")}
BLOCK_ATOMS = ("cut", "over", "bck", "word", "stored_over")
# (first, second) blocks of the edge shapes' pairs, on both sides of the 64-entry groups.  A frame of 64 blocks has no block 64:
# it gets its two last blocks and its two ends, so that the one-wave finish (at most 64 blocks) sees two flaws as well
EDGE_PAIRS = [(0, 64), (63, 64), (64, 65), (63, 128), (127, 128), (1, 129)]
EDGE64_PAIRS = [(0, 63), (62, 63)]
# LZ4F error numbers (frame_edges.ERROR_NAMES has the names)
(OK, GENERIC, MAXBLOCK, BLOCKCK, DSTSMALL, INCOMPLETE, FRAMESIZE, HEADERCK, CONTENTCK) = (0, 1, 2, 7, 11, 12, 14, 17, 18)

Piece = collections.namedtuple("Piece", "word payload ck out")      # a block as it stands in the frame; out: what it decodes to (None: it does not)
Case = collections.namedtuple("Case", "name shape mode flaws frame n_blocks content outs room")
#   flaws: ((atom, block or None), ...); n_blocks / content / outs: the shape's blocks, what the clean frame decodes to, and each
#   clean block's size; room: the block the window ends in (None: the windows are the test's)


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def _le32(v: int) -> bytes:
    return struct.pack("<I", v & 0xFFFFFFFF)


# ---- the blocks ----------------------------------------------------------------------------------------------------------------
def _taken(fr: Frame, body_at: int, out_at: int) -> Piece:
    seg = bytes(fr.body[body_at:])
    return Piece(struct.unpack("<I", seg[:4])[0], seg[4:-4], struct.unpack("<I", seg[-4:])[0], bytes(fr.out[out_at:]))


def _short(b, i: int, linked: bool):
    L = 6 + i % 5
    b.s(L, 8, L + 3 if linked and i else 3)                       # (linked, behind the first block: three bytes of the block in front)
    return b.s(10, 12, 7).s(3, 5, 1)


@functools.lru_cache(maxsize=None)
def clean_blocks(shape: str, mode: str) -> "tuple[Piece, ...]":
    n, kind = SHAPES[shape]
    fr = Frame(BSID, linked=mode == "linked", bck=True, cck=True, rng=_rng("flaw_pairs/%s/%s" % (shape, mode)))
    out = []
    for i in range(n):
        at, oat = len(fr.body), len(fr.out)
        b = fr.block()
        if kind == "short": _short(b, i, fr.linked).end(12)
        else: _fill(b, kind, BS - 20).end(20)
        out.append(_taken(fr, at, oat))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flawed_block(shape: str, mode: str, i: int, atom: str) -> Piece:
    """Block i of the shape with a flaw of its own payload (cut, over, stored_over), the clean blocks in front of it."""
    kind = SHAPES[shape][1]
    fr = Frame(BSID, linked=mode == "linked", bck=True, cck=True, rng=_rng("flaw_pairs/%s/%s/%d/%s" % (shape, mode, i, atom)))
    fr.out = bytearray(b"".join(p.out for p in clean_blocks(shape, mode)[:i]))
    oat = len(fr.out)
    if atom == "stored_over":
        fr.stored(fr.rng.integers(0, 256, BS + 1, dtype="uint8").tobytes())
    else:
        b = fr.block()
        if atom == "cut":
            (_short(b, i, fr.linked) if kind == "short" else _fill(b, kind, BS - 64)).raw(b"\x50abcd").close()
        elif kind == "short":
            b.s(8, BS - 19, 1).end(12)                                # over: 8 + (BS - 19) + 12 bytes
        else:
            _fill(b, kind, BS + 1 - 20).end(20)
    return _taken(fr, 0, oat)._replace(out=None)


# ---- the names -----------------------------------------------------------------------------------------------------------------
def _flaw_name(f) -> str:
    return f[0] if f[1] is None else "%s@%d" % f


def _parse(text: str):
    if text == "clean": return ()
    out = []
    for t in text.split("+"):
        a, _, b = t.partition("@")
        out.append((a, int(b) if b else None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def names() -> "tuple[str, ...]":
    out, seen = [], set()

    def add(shape, mode, *flaws):
        nm = "%s/%s/%s" % (shape, mode, "+".join(_flaw_name(f) for f in flaws) or "clean")
        if nm not in seen:
            seen.add(nm); out.append(nm)

    def pair(shape, mode, a, b):
        add(shape, mode, a, b); add(shape, mode, a); add(shape, mode, b)

    for mode in MODES:
        sh = "short5"
        add(sh, mode)
        for a in BLOCK_ATOMS:
            for b in BLOCK_ATOMS:
                pair(sh, mode, (a, 1), (b, 3))
        pair(sh, mode, ("bck", 1), ("cut", 1))
        pair(sh, mode, ("bck", 1), ("over", 1))
        behind = [("trunc.pay", 3), ("trunc.bck", 3), ("trunc.word", 3), ("trunc.end", None), ("trunc.cck", None), ("room", 3),
                  ("csize", None), ("cck", None)]
        for a in BLOCK_ATOMS:
            for f in behind:
                pair(sh, mode, (a, 1), f)
        for f in (("trunc.pay", 1), ("trunc.bck", 1), ("trunc.word", 1), ("room", 1)):
            for a in BLOCK_ATOMS:
                pair(sh, mode, f, (a, 3))
        pair(sh, mode, ("csize", None), ("cck", None))
        pair(sh, mode, ("room", 3), ("cck", None))
        pair(sh, mode, ("trunc.pay", 3), ("csize", None))
        for sh in ("full3s", "full3d"):
            add(sh, mode)
            for a in BLOCK_ATOMS:
                for b in BLOCK_ATOMS:
                    pair(sh, mode, (a, 0), (b, 2))
        for sh in ("edge64", "edge65", "edge130"):
            add(sh, mode)
            for i, j in (EDGE64_PAIRS if sh == "edge64" else EDGE_PAIRS):
                if j < SHAPES[sh][0]:
                    pair(sh, mode, ("bck", i), ("cut", j))
                    pair(sh, mode, ("cut", i), ("bck", j))
    return tuple(out)


def is_pair(c: Case) -> bool:
    return len(c.flaws) == 2


def parts(c: Case) -> "tuple[str, str]":
    """The names of a pair's two flaws alone."""
    return tuple("%s/%s/%s" % (c.shape, c.mode, _flaw_name(f)) for f in c.flaws)


def block_pair(c: Case) -> bool:
    """One of the 25 ordered pairs of block atoms at two different blocks."""
    return is_pair(c) and all(a in BLOCK_ATOMS for a, _ in c.flaws) and c.flaws[0][1] != c.flaws[1][1]


# ---- the frames ----------------------------------------------------------------------------------------------------------------
def _header(csize, linked: bool) -> bytes:
    flg = (1 << 6) | ((0 if linked else 1) << 5) | (1 << 4) | (1 << 2) | (8 if csize is not None else 0)
    h = bytes([flg, BSID << 4]) + (struct.pack("<Q", csize) if csize is not None else b"")
    return _le32(0x184D2204) + h + bytes([(oracle.xxh32(h) >> 8) & 0xFF])


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    shape, mode, text = name.split("/")
    flaws = _parse(text)
    clean = clean_blocks(shape, mode)
    pieces = list(clean)
    linked = mode == "linked"
    for a, i in flaws:                                                # the flaws of a payload first, then the words around it
        if a in ("cut", "over", "stored_over"): pieces[i] = flawed_block(shape, mode, i, a)
    for a, i in flaws:
        if a == "bck": pieces[i] = pieces[i]._replace(ck=pieces[i].ck ^ 1)
        if a == "word": pieces[i] = pieces[i]._replace(word=BS + 1, out=None)
    content = sum(len(p.out) for p in clean)
    atoms = [a for a, _ in flaws]
    f = bytearray(_header(content + 1 if "csize" in atoms else None, linked))
    at = []                                                           # per block: where its size word, payload and checksum word are
    for p in pieces:
        at.append((len(f), len(f) + 4, len(f) + 4 + len(p.payload)))
        f += _le32(p.word) + p.payload + _le32(p.ck)
    end = len(f)
    f += _le32(0) + _le32(oracle.xxh32(b"".join(p.out for p in pieces if p.out is not None)))
    if "cck" in atoms: f[-1] ^= 0x80
    room = None
    for a, i in flaws:
        if a == "trunc.pay": del f[at[i][1] + (at[i][2] - at[i][1]) // 2:]
        elif a == "trunc.bck": del f[at[i][2] + 2:]
        elif a == "trunc.word": del f[at[i][0] + 2:]
        elif a == "trunc.end": del f[end:]
        elif a == "trunc.cck": del f[len(f) - 2:]
        elif a == "room": room = i
    return Case(name, shape, mode, flaws, bytes(f), len(clean), content, tuple(len(p.out) for p in clean), room)


def cases() -> "list[Case]":
    return [case(n) for n in names()]


def room_window(c: Case, placed: bool) -> int:
    """The window of a room@b case: it ends in the middle of block b's output - behind the blocks in front of it, or, where a
    call gives every block of an independent frame its provisional place, at b * maxBlockSize."""
    b = c.room
    return (b * BS if placed and c.mode == "indep" else sum(c.outs[:b])) + c.outs[b] // 2


def windows(c: Case, placed: bool) -> "list[int]":
    """The windows a one-shot call is given: the content, five bytes more, every block's full room; a room@b case: its own."""
    if c.room is not None: return [room_window(c, placed)]
    return [c.content, c.content + 5, c.n_blocks * BS]


def ample(c: Case) -> int:
    return (c.n_blocks + 1) * BS


# ---- liblz4's recorded answers ---------------------------------------------------------------------------------------------------
BLOCK_FAILED = ("ERROR_GENERIC", "ERROR_decompressionFailed")       # liblz4 1.9.3's two names for a block that does not decode


@functools.lru_cache(maxsize=None)
def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def ref_verdict(rec: dict) -> str:
    """One recorded feed (fixture[name]["once"] or ["pieces"]) as one word: an error's name (the two names of a failed block as
    one), STALL_input / STALL_room where liblz4 only waits for more, or OK:<the output's SHA-256>."""
    if rec["error"]: return "ERROR_blockFailed" if rec["error"] in BLOCK_FAILED else rec["error"]
    if rec["stall"]: return "STALL_" + rec["stall"]
    return "OK:" + rec["out_sha256"]


def pieces_seed(c: Case) -> int:
    return zlib.crc32(c.name.encode())


def feed(L, frame: bytes, budget: int, seed=None) -> dict:
    """LZ4F_decompress of the library L (liblz4 when the fixture is minted, this project's when it is tested) until the frame ends,
    an error, or a call that neither takes input nor gives output: whole (seed None: the whole frame and all the room per call) or in
    pieces of 1..300 bytes of input and 1..500 bytes of room, `budget` bytes of room in all -> what the fixture records per feed, and
    "out": the bytes that came out."""
    import numpy as np
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    rng = np.random.default_rng(seed) if seed is not None else None
    d = vp()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(d), 100))
    src = ctypes.create_string_buffer(frame, max(len(frame), 1))
    dst = ctypes.create_string_buffer(max(budget, 1) if rng is None else 512)
    out, pos = bytearray(), 0
    rec = {"error": None, "stall": None, "out_sha256": None}
    try:
        while True:
            sn, dn = (int(rng.integers(1, 301)), int(rng.integers(1, 501))) if rng is not None else (len(frame), budget)
            ss, ds = sz(min(sn, len(frame) - pos)), sz(min(dn, budget - len(out)))
            r = L.LZ4F_decompress(d, dst, ctypes.byref(ds), ctypes.byref(src, pos), ctypes.byref(ss), None)
            if L.LZ4F_isError(r):
                rec["error"] = L.LZ4F_getErrorName(r).decode()
                break
            out += dst.raw[:ds.value]; pos += ss.value
            if r == 0:
                rec["out_sha256"] = sha(out)
                break
            if ss.value == 0 and ds.value == 0:
                rec["stall"] = "room" if len(out) == budget else "input"
                break
    finally:
        L.LZ4F_freeDecompressionContext(d)
    return rec


def oracle_verdict(c: Case) -> str:
    """The oracle's one-shot answer in ref_verdict's words: its frameHeader_incomplete is the streaming API's wait for input, its
    dstMaxSize_tooSmall the wait for room (oracle/orc_lz4frame.c says so)."""
    win = room_window(c, False) if c.room is not None else ample(c)
    try:
        out, _ = oracle.decompress_frame(c.frame, cap=win)
    except oracle.OracleError as e:
        nm = str(e)
        return {"ERROR_frameHeader_incomplete": "STALL_input", "ERROR_dstMaxSize_tooSmall": "STALL_room"}.get(
            nm, "ERROR_blockFailed" if nm in BLOCK_FAILED else nm)
    return "OK:" + sha(out)


# ---- the written order -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4096)
def lz4_block(p: bytes, room: int, hist: bytes):
    """A compressed block's payload decoded into `room` bytes with `hist` in front -> the bytes, or None: the block grammar of
    lz4_grammar's docstring (literal runs, the last-sequence rules, 0 < offset <= bytes in front, a match ends 5 bytes before room)."""
    n = len(p)
    if n == 0: return None
    out, h, ip = bytearray(hist), len(hist), 0
    while True:
        if ip >= n: return None
        tok = p[ip]; ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                if ip >= n: return None
                s = p[ip]; ip += 1; lit += s
                if s != 255: break
        in_left, out_left = n - ip, room - (len(out) - h)
        if lit + 12 > out_left or lit + 8 > in_left:                 # must be the last sequence
            if lit != in_left or lit > out_left: return None
            out += p[ip:ip + lit]
            return bytes(out[h:])
        out += p[ip:ip + lit]; ip += lit
        off = p[ip] | (p[ip + 1] << 8); ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                if ip >= n: return None
                s = p[ip]; ip += 1; ml += s
                if ip + 4 >= n: return None
                if s != 255: break
        ml += 4
        if off == 0 or off > len(out) or ml + 5 > room - (len(out) - h): return None
        src = len(out) - off
        if off >= ml: out += out[src:src + ml]
        else: out += (bytes(out[src:]) * (ml // off + 1))[:ml]


def block_fail_status(kind: int, at: int, win: int) -> int:
    """A block that failed at `at` in a window of `win` bytes.  kind -2: it decodes, but not into its room; -3: not even with a
    whole block of room; -1: not into the room it had.  Less room than a whole block is "the output does not fit"."""
    short_room = at <= win and win - at < BS and kind != -3
    return DSTSMALL if kind == -2 or short_room else GENERIC


def failures(frame: bytes, window: int, placed: bool = True, decode_first: bool = False) -> "list[tuple[int, int]]":
    """Every failure the written order names for this span and window, IN that order: [(status, first_bad_block)].  The verdict
    is the first of them; what comes behind it is there for the tests that show a wrong chooser is caught.
    placed: the device-pointer calls' placement - block b of any frame has its provisional place at b * maxBlockSize, which the
    walk wants inside the window; an independent block is decoded there, a linked one behind its predecessors, into what is left of
    the window up to maxBlockSize; the frame's last block with less than a block of room is judged against a whole block when the
    window is no multiple of maxBlockSize.  Not placed (the host-pointer call): blocks lie back to back, each is judged against
    maxBlockSize and must then fit what is left."""
    out, n = [], len(frame)
    # 1. the span and the offsets: the caller's
    # 2. the header
    if n < 7: return [(INCOMPLETE, NONE)]
    flg = frame[4]
    hs = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    assert frame[:4] == _le32(0x184D2204) and flg >> 6 == 1 and not flg & 2 and frame[5] == BSID << 4, "this corpus has no header flaw but csize"
    if n < hs: return [(INCOMPLETE, NONE)]
    if (oracle.xxh32(frame[4:hs - 1]) >> 8) & 0xFF != frame[hs - 1]: return [(HEADERCK, NONE)]
    bck, linked = 4 if flg & 0x10 else 0, not flg & 0x20
    # 3. the walk: every size word from first to last, before any block is looked at
    pos, blocks, walk = hs, [], OK
    while True:
        if n - pos < 4: walk = INCOMPLETE; break
        w = struct.unpack_from("<I", frame, pos)[0]; pos += 4
        if w == 0: break
        csz = w & 0x7FFFFFFF
        if csz > BS: walk = MAXBLOCK; break
        if n - pos < csz + bck: walk = INCOMPLETE; break
        if placed and len(blocks) * BS >= window: walk = DSTSMALL; break
        blocks.append((w, pos)); pos += csz + bck
    if walk == OK and flg & 4 and n - pos < 4: walk = INCOMPLETE
    if walk: out.append((walk, NONE))
    # 4. the blocks in order, each block's checksum before its decode
    done, hist, gots = 0, b"", []
    for b, (w, at_src) in enumerate(blocks):
        csz = w & 0x7FFFFFFF
        payload = frame[at_src:at_src + csz]
        here = []
        if bck and oracle.xxh32(payload) != struct.unpack_from("<I", frame, at_src + csz)[0]: here.append((BLOCKCK, b))
        at = b * BS if placed and not linked else done
        left = max(window - at, 0)
        room = min(left, BS) if placed else BS
        kind, got = 0, b""
        if w >> 31:
            if csz > min(left, BS): kind = -2
            else: got = payload
        else:
            got = lz4_block(payload, room, hist if linked else b"")
            if got is None and placed and b + 1 == len(blocks) and window % BS and left < BS:
                got = lz4_block(payload, BS, hist if linked else b"")
                kind = -3 if got is None else 0
            elif got is None: kind = -1
            if got is not None and len(got) > left: kind = -2
        if kind:
            here.append((block_fail_status(kind, at, window) if placed else DSTSMALL if kind == -2 else GENERIC, b))
            got = b""
        out += here[::-1] if decode_first else here
        done += len(got); gots.append(got)
        hist = (hist + got)[-65536:]
    # 5. the content size, 6. the content checksum (over what the blocks gave; only a frame whose size words walk has an end)
    if walk == OK:
        if flg & 8 and struct.unpack_from("<Q", frame, 6)[0] != done: out.append((FRAMESIZE, NONE))
        if flg & 4 and oracle.xxh32(b"".join(gots)) != struct.unpack_from("<I", frame, pos)[0]: out.append((CONTENTCK, NONE))
    return out


def one_shot_verdict(c: Case, window: int, placed: bool = True, rule: str = "first") -> "tuple[int, int]":
    """(status, first_bad_block) of a one-shot call on this case's frame and `window` bytes: the first failure in the written
    order.  rule "last" (the last failure wins) and "decode_first" (a block's decode failure beats its checksum) are the two wrong
    choosers the CPU test shows the comparison catches."""
    fs = failures(c.frame, window, placed, decode_first=rule == "decode_first")
    if not fs: return (OK, NONE)
    return fs[-1] if rule == "last" else fs[0]


# ---- the comparison the GPU tests use ------------------------------------------------------------------------------------------
def disagreements(rows) -> list:
    """rows: (case name, entry point, (status, first_bad_block) the call gave, the model's, later_ok) -> the rows that disagree.
    later_ok: the stated exception - the single call on a malformed LINKED frame may name a later block of the same frame: the
    same status, and a first_bad_block that is not in front of the model's."""
    bad = []
    for name, entry, got, want, later_ok in rows:
        same = tuple(got) == tuple(want)
        if not same and later_ok and got[0] == want[0] != OK and want[1] != NONE and got[1] != NONE and got[1] >= want[1]: same = True
        if not same: bad.append((name, entry, tuple(got), tuple(want)))
    return bad
