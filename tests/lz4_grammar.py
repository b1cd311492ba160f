"""The LZ4 block grammar's edges as a corpus of named frames (test helper, not a test module).

Every decoder path of this library parses sequences itself and makes its own bounds checks.  The encoders the rest of the
suite uses (liblz4's fast one, this library's own) never write the shapes liblz4's LZ4_decompress_safe only just accepts or
only just rejects; this module writes them on purpose, deterministically, so that oracle/mint_golden.py can record liblz4's
verdict on each (tests/golden/grammar.json) and the tests can hold the oracle and every GPU path to it.

The checks being probed (oracle/orc_lz4block.c restates them; room = the frame's maxBlockSize, hist = history in front):
  - a literal run with lit + 12 > room - op or lit + 8 > in_left must be the block's last: it ends exactly at the payload end;
  - a match needs 0 < offset <= op + hist, its length bytes must stop before iend - 4, and it must end at least 5 bytes
    before room;
  - a block's payload is at most maxBlockSize, a stored one too.

Families (the name's first word):
  end       a block's last sequences: literals L, match M (0..6 length bytes), final literals k, in a short (last) block and in
            a block that decodes to exactly room (d = 0) or room + 1 - the last-accepted / first-rejected pairs of every rule
            that looks at the end of the block or the payload
  lit       literal runs of 0, 14, 15, 269, 270, 65836 bytes, as a block's first sequence and in its middle; a cut extension
  off       offsets 1..16, 31..33, 63..65, 127, 128, 65535 with match lengths 4, 19, 64, 1000, 70000; op + hist and one more
  mext      match-length extensions of 255s at every alignment against the 8-byte words the parsers fetch
  lext      literal-length extensions likewise, on both sides of what one 8-byte fetch decides (7 length bytes)
  link      linked frames: history from one full block, 2-4 short blocks, a stored block; op + hist and one more
  blk       payload of exactly maxBlockSize and one byte more; stored blocks of maxBlockSize and one byte more; a 1-byte payload
            (0x00) and short blocks in the middle of a frame; block and content checksums
  carrier   64 KiB .. 4 MiB independent and 64 KiB / 4 MiB linked framings of sparse (~1 KiB sequences: the self-index and
            indexed decoders) and dense (~13-byte sequences: the relay / wave-per-block decoders) blocks with the patterns
            above planted as a block's first sequence, at its end, straddling 64-byte payload windows and spread over the
            block so that the stretch starts of the stretch-parallel self-index fall on them
Frames are rebuilt identically from the case name on any machine (numpy's PCG64 seeded by the name's CRC32).

This corpus aims at parsers and bounds checks.  Copy DEPENDENCIES - when a match may be copied and where its bytes come from, in
every decoder - live in match_dep_cases.py, which builds on Frame / Block / lz4_seq of this module.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

KB64 = 65536


def ext(v: int) -> bytes:
    out = bytearray()
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)
    return bytes(out)


def lz4_seq(lit: bytes, mlen: int, off: int) -> bytes:
    """One LZ4 sequence (token, literal length bytes, literals, offset, match length bytes); mlen == 0: the block's last, literals only."""
    ll, ml = len(lit), (mlen - 4 if mlen else 0)
    b = bytearray([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15: b += ext(ll - 15)
    b += lit
    if mlen:
        b += bytes([off & 255, off >> 8])
        if ml >= 15: b += ext(ml - 15)
    return bytes(b)


def _xxh32(b: bytes) -> int:
    import oracle
    return oracle.xxh32(b)


class Frame:
    """An LZ4 frame built block by block; `out` is what it is meant to decode to (for accepted cases: what it decodes to)."""

    def __init__(self, bsid: int, linked: bool = False, bck: bool = False, cck: bool = False, rng=None):
        self.bsid, self.bs, self.linked, self.bck, self.cck = bsid, 1 << (8 + 2 * bsid), linked, bck, cck
        self.out = bytearray()
        self.body = bytearray()
        self.rng = rng
        self.short_mid = False                          # a block shorter than maxBlockSize that is not the last
        self._last_short = False
        self.planted = []                               # per block: its sequences as written (in_off, out_pos, lit, mlen, off); None: stored or raw

    def header(self) -> bytes:
        flg = (1 << 6) | ((0 if self.linked else 1) << 5) | (int(self.bck) << 4) | (int(self.cck) << 2)
        bd = (self.bsid & 7) << 4
        h = bytes([flg, bd])
        return struct.pack("<I", 0x184D2204) + h + bytes([(_xxh32(h) >> 8) & 0xFF])

    def _emit(self, word: int, payload: bytes, produced: int):
        if self._last_short: self.short_mid = True
        self._last_short = produced < self.bs
        self.body += struct.pack("<I", word) + payload
        if self.bck: self.body += struct.pack("<I", _xxh32(payload))

    def block(self) -> "Block":
        return Block(self)

    def stored(self, data: bytes, word_size: int | None = None):
        self.planted.append(None)
        self._emit((len(data) if word_size is None else word_size) | 0x80000000, data, len(data))
        self.out += data

    def raw_block(self, payload: bytes, produced: int, word: int | None = None, seqs=None):
        self.planted.append(seqs)
        self._emit(len(payload) if word is None else word, payload, produced)

    def bytes(self) -> bytes:
        tail = struct.pack("<I", 0)
        if self.cck: tail += struct.pack("<I", _xxh32(bytes(self.out)))
        return self.header() + bytes(self.body) + tail


class Block:
    """Sequences of one compressed block; the output is tracked as liblz4 would produce it (zeros where a match has no source)."""

    def __init__(self, fr: Frame):
        self.fr, self.start, self.body = fr, len(fr.out), bytearray()
        self.seqs = []                                  # (payload offset of the token, output position, literals, match length, offset)

    @property
    def op(self) -> int:
        return len(self.fr.out) - self.start

    @property
    def reach(self) -> int:                             # the largest offset the decoder accepts here: op + hist
        hist = min(self.start, KB64) if self.fr.linked else 0
        return self.op + hist

    def lits(self, n: int) -> bytes:
        return self.fr.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def s(self, lit, mlen: int, off: int):
        lit = self.lits(lit) if isinstance(lit, int) else lit
        if self.seqs is not None: self.seqs.append((len(self.body), self.op, len(lit), mlen, off))
        self.body += lz4_seq(lit, mlen, off)
        out = self.fr.out
        out += lit
        if 0 < off <= self.reach:
            src = len(out) - off
            if off >= mlen: out += out[src:src + mlen]
            else:
                pat = bytes(out[src:src + off])
                out += (pat * (mlen // off + 1))[:mlen]
        else:
            out += bytes(mlen)
        return self

    def raw(self, b: bytes):
        self.seqs = None                                # (hand-made bytes: no planted list for this block)
        self.body += b
        return self

    def end(self, lit=0, word: int | None = None):
        lit = self.lits(lit) if isinstance(lit, int) else lit
        if self.seqs is not None: self.seqs.append((len(self.body), self.op, len(lit), 0, 0))
        self.body += lz4_seq(lit, 0, 0)
        self.fr.out += lit
        self.close(word)

    def close(self, word: int | None = None):
        self.fr.raw_block(bytes(self.body), self.op, word, self.seqs if word is None else None)

    # ---- fillers: sequences up to `target` output bytes of this block
    def sparse(self, target: int):
        """~1 KiB sequences: 600 literals and a 424-byte copy from 600 back (what the self-index / indexed decoders are for)."""
        while self.op + 1024 + 64 <= target:
            self.s(600, 424, 600)
        return self.pad(target)

    def dense(self, target: int):
        """~13-byte sequences: 1..9 literals and a 4..18-byte match from anywhere in reach (the relay / wave-per-block decoders)."""
        rng = self.fr.rng
        if self.op < 64 and target - self.op > 128: self.s(64 - self.op, 4, 1)
        n = target - 64 - self.op
        if n > 0:
            ll = rng.integers(1, 10, n // 8 + 1)
            ml = rng.integers(4, 19, n // 8 + 1)
            r = rng.random(n // 8 + 1)
            i = 0
            while self.op + 64 <= target:
                reach = min(self.reach, 65535)
                l, m = int(ll[i]), int(ml[i])
                off = 1 + int(r[i] * reach) if r[i] > 0.1 else 1 + int(r[i] * 30) % reach     # (a tenth of them near: overlapping copies)
                self.s(l, m, off)
                i += 1
        return self.pad(target)

    def pad(self, target: int):
        """One sequence that brings the output to exactly `target` (>= 4 bytes away)."""
        gap = target - self.op
        assert gap >= 4 or gap == 0, gap
        assert gap == 0 or self.reach + gap - 4 >= 1
        if gap: self.s(gap - 4, 4, 1)
        return self


# ------------------------------------------------------------------------------------------------------------------------
def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _fill(b: Block, kind: str, target: int):
    return b.sparse(target) if kind == "sparse" else b.dense(target)


def mlen_with_ext(e: int) -> int:
    """A match length whose encoding has exactly e length bytes (e = 0: none)."""
    return 15 if e == 0 else 4 + 15 + 255 * (e - 1) + 7


def lit_with_ext(e: int, last: int) -> int:
    """A literal length whose encoding has exactly e length bytes (e >= 1), the last one `last` (0..254)."""
    return 15 + 255 * (e - 1) + last


END_M = [4, 8, 18, 19, mlen_with_ext(2), mlen_with_ext(5), mlen_with_ext(6)]
END_K = [0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13]


def _end_case(name, kind, full, L, M, k, d=0, bsid=4):
    fr = Frame(bsid, rng=_rng(name))
    b = fr.block()
    tail = L + M + k
    total = fr.bs + d if full else 3000 + (len(name) % 7)
    off = [1, 3, 17, 600][(L + M + k) % 4]
    _fill(b, kind, total - tail)
    b.s(L, M, off).end(k)
    return fr


def _frames():
    """(name, Frame) for every case."""
    # ---- end shapes: short last block and block of exactly room (+1)
    for kind in ("sparse", "dense"):
        for M in END_M:
            for k in END_K:
                for full in (False, True):
                    nm = "end/%s/%s/M%d/k%d" % (kind, "full" if full else "short", M, k)
                    yield nm, _end_case(nm, kind, full, 3, M, k)
        for L in (0, 1, 4, 5, 12, 13, 16, 300):
            for k in (5, 8):
                for M in (4, 7):
                    nm = "end/%s/full/L%d/M%d/k%d" % (kind, L, M, k)
                    yield nm, _end_case(nm, kind, True, L, M, k)
        for d in (-1, 1):
            nm = "end/%s/full_d%+d/M8/k5" % (kind, d)
            yield nm, _end_case(nm, kind, True, 3, 8, 5, d)
        for bsid in (5, 7):                                          # room is the frame's block size, not 64 KiB
            for M, k in ((4, 0), (4, 4), (4, 5), (4, 7), (4, 8), (8, 4), (8, 5)):
                for full in (False, True):
                    if full and bsid == 7 and (kind == "dense" or k == 0):
                        continue                                 # (4 MiB each: the dense pairs are the 256 KiB ones' boundary)
                    nm = "end/%s/%s/bsid%d/M%d/k%d" % (kind, "full" if full else "short", bsid, M, k)
                    yield nm, _end_case(nm, kind, full, 3, M, k, 0, bsid)
    # a non-last literal run with lit + 12 == room - op (accepted) and one literal more (rejected), in a block of room
    for extra in (0, 1):
        for L in (40, 300):
            nm = "end/lit12/L%d/+%d" % (L, extra)
            fr = Frame(4, rng=_rng(nm)); b = fr.block()
            b.dense(fr.bs - L - 12); b.s(L + extra, 4, 8).end(8 - extra)
            yield nm, fr
    # ---- literal runs
    for L in (0, 14, 15, 16, 269, 270, 271, 524, 525, 65836):
        for where in ("first", "mid"):
            nm = "lit/%s/L%d" % (where, L)
            fr = Frame(5, rng=_rng(nm)); b = fr.block()
            if where == "mid": b.dense(5000)
            b.s(L, 4, 8 if (L >= 8 or where == "mid") else max(L, 1))
            b.dense(b.op + 4000).end(20)
            yield nm, fr
    for nm, tail in (("lit/cut/ext_missing", b"\xf0"), ("lit/cut/ext_255_at_end", b"\xf0\xff"),
                     ("lit/cut/ext_255_255", b"\xf0\xff\xff"), ("lit/cut/short_by_one", b"\x50abcd"),
                     ("lit/cut/long_by_one", b"\x50abcdef"), ("lit/cut/offset_cut", b"\x14abc\x01"),
                     ("lit/cut/token_only", b"\x14")):
        fr = Frame(4, rng=_rng(nm)); b = fr.block(); b.dense(2000); b.raw(tail).close()
        yield nm, fr
    # ---- offsets x match lengths, valid: one frame per match length, in 256 KiB, 1 MiB and 4 MiB blocks
    OFFS = list(range(1, 17)) + [31, 32, 33, 63, 64, 65, 127, 128, 65535]
    for M in (4, 19, 64, 1000, 70000):
        bsid = 7 if M == 70000 else 5
        nm = "off/sweep/M%d" % M
        fr = Frame(bsid, rng=_rng(nm)); b = fr.block()
        b.dense(KB64 + 100)
        for i, off in enumerate(OFFS):
            b.s(i % 9, M, off)
            b.sparse(b.op + 2100) if i % 2 else b.dense(b.op + 300)
        b.end(30)
        yield nm, fr
    # op + hist (a source at the very start of the block) and one more, independent, as first sequence and mid-block
    for where, pre in (("first", 0), ("mid", 5000)):
        for L in (4, 20):
            for extra in (0, 1):
                nm = "off/reach/%s/L%d/+%d" % (where, L, extra)
                fr = Frame(4, rng=_rng(nm)); b = fr.block()
                if pre: b.dense(pre)
                b.s(L, 8, b.op + L + extra); b.dense(b.op + 300).end(10)
                yield nm, fr
    for where in ("first", "mid"):
        nm = "off/zero/%s" % where                       # offset 0: liblz4 1.9.3 accepts it (copies bytes nobody wrote); rejected here
        fr = Frame(4, rng=_rng(nm)); b = fr.block()
        if where == "mid": b.dense(3000)
        b.s(40, 8, 0); b.dense(b.op + 300).end(10)
        yield nm, fr
    # ---- match-length extensions across the parsers' 8-byte words: every alignment, 1..10 length bytes
    for align in range(8):
        nm = "mext/align%d" % align
        fr = Frame(4, rng=_rng(nm)); b = fr.block(); b.dense(1000)
        for e in range(1, 11):
            b.s(align + (e % 3) * 8, mlen_with_ext(e), 1 + e * 3)
            b.s(align, 4, 7)
        b.dense(b.op + 200).end(12)
        yield nm, fr
    # ---- linked frames
    for bsid in (4, 7):
        for hist_blocks, stored in (((), False), (("full",), False), ((100, 200), False), ((10, 20, 30, 40), False),
                                    ((1000, 3000, 7), False), ((500,), True), ((40000,), True)):
            if bsid == 7 and hist_blocks == ("full",):
                continue                                         # (a full 4 MiB block of history says no more than a 64 KiB one)
            for extra in (0, 1):
                tag = ("stored" if stored else "") + ("+".join(str(h) for h in hist_blocks) or "none")
                nm = "link/bsid%d/hist_%s/+%d" % (bsid, tag, extra)
                fr = Frame(bsid, linked=True, rng=_rng(nm))
                for h in hist_blocks:
                    if stored: fr.stored(fr.rng.integers(0, 256, h, dtype=np.uint8).tobytes())
                    elif h == "full": b = fr.block(); b.dense(fr.bs - 20); b.end(20)
                    else: fr.block().end(h)                  # a short block of literals only
                b = fr.block()
                if hist_blocks == ("full",):                 # full history: the farthest offset, and a match that spans blocks
                    b.s(6, 3000 + extra, 65535).s(3, 70, 65530 - extra)
                else:
                    b.s(6, 40 + 3 * extra, b.reach + 6 + extra)
                b.dense(b.op + 500).end(9)
                yield nm, fr
    for bsid in (4, 7):                                      # matches whose source spans several short blocks
        nm = "link/bsid%d/span" % bsid
        fr = Frame(bsid, linked=True, rng=_rng(nm))
        for h in (3000, 2000, 1000, 5000):
            b = fr.block(); b.dense(h - 12); b.end(12)
        b = fr.block(); b.s(2, 9000, 10990).s(1, 200, 64).s(0, 6000, 11000)
        b.dense(b.op + 2000).end(6)
        yield nm, fr
    # ---- blocks
    for bsid in (4, 5):
        bs = 1 << (8 + 2 * bsid)
        for extra in (0, 1):
            nm = "blk/payload_bs/bsid%d/+%d" % (bsid, extra)      # a compressed block whose size word is bs (+1): one literal run
            fr = Frame(bsid, rng=_rng(nm))
            n = bs + extra
            el = 1
            while len(lz4_seq(bytes(n - 1 - el), 0, 0)) != n: el += 1
            fr.block().end(n - 1 - el)
            yield nm, fr
            nm = "blk/stored_bs/bsid%d/+%d" % (bsid, extra)
            fr = Frame(bsid, rng=_rng(nm))
            fr.stored(fr.rng.integers(0, 256, bs + extra, dtype=np.uint8).tobytes())
            b = fr.block(); b.dense(1000); b.end(5)
            yield nm, fr
    for linked in (False, True):
        for bck, cck in ((0, 0), (1, 1)):
            nm = "blk/%s/one_byte_payload/bck%d_cck%d" % ("linked" if linked else "indep", bck, cck)
            fr = Frame(4, linked=linked, bck=bool(bck), cck=bool(cck), rng=_rng(nm))
            b = fr.block(); b.dense(fr.bs - 16); b.end(16)
            fr.raw_block(b"\x00", 0)
            b = fr.block(); b.dense(9000); b.end(7)
            yield nm, fr
            nm = "blk/%s/short_mid/bck%d_cck%d" % ("linked" if linked else "indep", bck, cck)
            fr = Frame(4, linked=linked, bck=bool(bck), cck=bool(cck), rng=_rng(nm))
            for n in (fr.bs, 1000, fr.bs, 33, fr.bs, 5000):
                b = fr.block(); _fill(b, "sparse" if n == 1000 else "dense", n - 12); b.end(12)
            yield nm, fr
    # ---- carriers: the patterns planted through big blocks of either kind, in every framing
    plant = [(3, 4, 1), (0, 4, 1), (0, 18, 3), (15, 19, 65535), (270, mlen_with_ext(5), 2), (0, 4, 65535), (9, 1000, 64)]
    for bsid, linked in ((4, False), (5, False), (6, False), (7, False), (4, True), (7, True)):
        for kind in ("sparse", "dense"):
            # (an end 4 bytes short of room is rejected: the whole frame is.  In 1 and 4 MiB blocks that verdict is one case, not four)
            for end_k in ((5, 4) if bsid <= 5 or (kind == "dense" and not linked and bsid == 7) else (5,)):
                nm = "carrier/%s%d/%s/k%d" % ("linked" if linked else "indep", bsid, kind, end_k)
                fr = Frame(bsid, linked=linked, bck=(bsid == 6), cck=(bsid == 5), rng=_rng(nm))
                bs = fr.bs
                nblk = 3 if bs <= (1 << 20) else 2
                step = max(bs // 16, 4096) + 37
                for i in range(nblk):
                    full = i < nblk - 1
                    b = fr.block()
                    b.s(*(plant[i % len(plant)] if linked and i else (8, 4, 8)))        # as a block's first sequence
                    j = 0
                    while b.op + step + 3000 < (bs - 4096 if full else bs // 3):
                        _fill(b, kind, b.op + step + j % 5)                          # at positions that drift against 64-byte windows
                        L, M, off = plant[j % len(plant)]
                        b.s(L, M, min(off, b.reach + L))
                        j += 1
                    if full:                                 # full blocks end exactly at room, the last match end_k bytes before it
                        _fill(b, kind, bs - end_k - 8 - 3); b.s(3, 8, 9).end(end_k)
                    else:                                    # the last block is short, in the other kind, end_k literals behind its last match
                        _fill(b, "dense" if kind == "sparse" else "sparse", b.op + min(50000, bs // 3)); b.s(3, 4, 9).end(end_k)
                yield nm, fr
    # many small blocks: a frame of over 1 MiB in 64 KiB blocks has its size words looked for in parallel
    nm = "carrier/indep4/many"
    fr = Frame(4, rng=_rng(nm))
    for i in range(40):
        b = fr.block(); b.s(8, 4, 8); b.dense(fr.bs - 8 - 4 - 8); b.s(8, 4, 1 + i).end(8)
    yield nm, fr
    # ---- literal-length extensions across the parsers' 8-byte words: every alignment, 1..10 length bytes (11 for the last run), the
    # last byte 0 and 254.  Seven bytes (6 x 0xFF and one more, L = 1545..1799) are the most one 8-byte read decides; from 7 x 0xFF
    # on (L >= 1800) the parsers go byte by byte.  (Behind all other families: slices of the corpus keep their picks.)
    for align in range(8):
        nm = "lext/align%d" % align
        fr = Frame(4, rng=_rng(nm)); b = fr.block(); b.dense(1000)
        for e in range(1, 11):
            for last in (0, 254):
                b.s(lit_with_ext(e, last), 4 + e % 3, 1 + e * 3)
                b.s(align, 4, 7)
        b.s(lit_with_ext(11, 0), 4, 9)                       # 15 + 255 * 10
        b.s(align, 4, 7)
        assert b.op + 300 <= fr.bs, b.op
        b.dense(b.op + 200).end(12)
        yield nm, fr


def corpus():
    """[(name, frame bytes, meta)] - meta: bs, linked, short_mid, content (bytes the frame is meant to decode to), planted (per
    block: the sequences as written, None for stored and hand-made blocks)."""
    out = []
    for name, fr in _frames():
        fb = fr.bytes()
        out.append((name, fb, dict(bs=fr.bs, linked=fr.linked, short_mid=fr.short_mid, content=len(fr.out), planted=fr.planted)))
    return out
