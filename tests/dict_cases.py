"""Shared-dictionary cases for the batch calls (test helper, not a test module; numpy + the oracle only).

The batch calls' `_usingDict` forms put one dictionary in front of every frame (linked blocks) or every block (independent
blocks), as liblz4's LZ4F_compressFrame_usingCDict / LZ4F_decompress_usingDict do.  This module rebuilds, from seeded
generators alone, everything tests/golden/dict_frames.json was minted from (tools/mint_dict_golden.py, which drives liblz4):
  - the dictionaries: 1 byte, 3 bytes, 1 KiB, 65 525 bytes (the phrase dictionary) and 200 000 bytes (only its tail counts);
  - the natural corpus: records stitched from phrases of the phrase dictionary with a few random bytes between them, of every
    length where the block format's end rules change (0, 1, 4, 5, 11, 12, 13, 17, 63..65, 255, 300, 1000, 4096; the other
    dictionaries get six of them), a verbatim slice
    of the dictionary, a record that begins with the dictionary's tail and repeats its own beginning behind it (liblz4 then
    writes a match that crosses the seam), more
    records of 17..4096 bytes for the phrase dictionary (the ratio test's corpus), and for the phrase dictionary records of
    65 535, 65 536, 65 537 and 131 085 bytes (linked frames, and independent frames of several 64 KiB blocks);
  - the planted frames: hand-built with lz4_grammar.lz4_seq and sealed, liblz4's verdict on each recorded in the fixture;
  - the dictionary model: the frame walked, every block through oracle.decompress_block with history = the dictionary's tail
    (plus the output so far when linked) - what the CPU test holds to liblz4's verdicts and the GPU test holds the device to.
The fixture stores the SHA-256 of every dictionary, input and planted frame: `check_sha` fails loudly where a regenerated one differs.
"""
from __future__ import annotations

import base64
import hashlib
import json
import os
import struct
import zlib

import numpy as np

import oracle
from lz4_grammar import Frame, lz4_seq

KB64 = 65536
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict_frames.json")
DICT_LEN = {"d1": 1, "d3": 3, "d1k": 1024, "phrase": 65525, "big": 200000}
MODES = ("indep", "linked")
SMALL = (0, 1, 4, 5, 11, 12, 13, 17, 63, 64, 65, 255, 300, 1000, 4096)
FEW = (0, 5, 13, 65, 300, 1000)                     # ... of the other dictionaries
BIG = (65535, 65536, 65537, 131085)
RATIO_MAX = 4096                                    # the ratio test's records: at most this long
N_EXTRA = 32                                        # more records of 17..4096 bytes, phrase dictionary only


def rng_of(name: str):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


_cache: dict = {}


def _phrase_stream(name: str, n: int) -> bytes:
    """n bytes of 'words': a pool of 900 phrases of 5..24 lower-case letters, drawn at random with a separator behind each."""
    r = rng_of("pool/" + name)
    pool = [bytes(r.integers(97, 123, int(k), dtype=np.uint8)) for k in r.integers(5, 25, 900)]
    out = bytearray()
    while len(out) < n:
        out += pool[int(r.integers(0, len(pool)))] + b" "
    return bytes(out[:n])


def dictionary(name: str) -> bytes:
    if name not in _cache:
        if name == "d1": d = b"x"
        elif name == "d3": d = b"abc"
        elif name == "d1k": d = dictionary("phrase")[-1024:]
        else: d = _phrase_stream(name, DICT_LEN[name])
        assert len(d) == DICT_LEN[name]
        _cache[name] = d
    return _cache[name]


def tail(d: bytes) -> bytes:
    return d[-KB64:]


def stitched(name: str, n: int, source: bytes, piece=(24, 96)) -> bytes:
    """n bytes: slices of `source` (piece[0]..piece[1] bytes each) with 0..2 random bytes between them."""
    r = rng_of("rec/" + name)
    out = bytearray()
    while len(out) < n:
        k = int(r.integers(piece[0], piece[1] + 1))
        at = int(r.integers(0, max(1, len(source) - k)))
        out += source[at:at + k]
        out += bytes(r.integers(0, 256, int(r.integers(0, 3)), dtype=np.uint8))
    return bytes(out[:n])


def _big_record(n: int, src: bytes) -> bytes:
    """n bytes that stay small in the fixture: 6000 stitched bytes over and over, a 600-byte slice of the dictionary every 15 000."""
    unit = stitched("b%d" % n, 6000, src, (1500, 6000))
    out = bytearray((unit * (n // len(unit) + 1))[:n])
    for i, p in enumerate(range(9000, n - 600, 15000)):
        out[p:p + 600] = src[i * 7001:i * 7001 + 600]
    return bytes(out)


def natural(dname: str) -> "list[tuple[str, bytes]]":
    """(name, input) of a dictionary's natural records.  The fixture has each as an independent frame, and those longer than a
    block as a linked frame too (liblz4 writes a single block as an independent one whatever was asked for)."""
    key = ("natural", dname)
    if key not in _cache:
        d, src = dictionary(dname), tail(dictionary("big" if dname == "big" else "phrase"))
        recs = [("n%d" % n, stitched("%s/n%d" % (dname, n), n, src)) for n in (SMALL if dname == "phrase" else FEW)]
        recs.append(("slice", d[len(d) // 3:len(d) // 3 + 700]))
        # (the dictionary's tail and then the record's own beginning again: a match that starts in the dictionary runs on across the seam)
        recs.append(("tail", d[-300:] + d[-300:-180] + stitched(dname + "/tail", 400, src)))
        if dname == "phrase":
            r = rng_of("extra")
            for k in range(N_EXTRA):
                n = int(np.exp(r.uniform(np.log(17), np.log(4096))))
                recs.append(("x%d_%d" % (k, n), stitched("x%d" % k, n, src)))
            recs += [("b%d" % n, _big_record(n, src)) for n in BIG]
        _cache[key] = recs
    return _cache[key]


# ---- frames: the walk and the dictionary model ----
def walk(frame: bytes) -> dict:
    """A frame's header and blocks: {flg, bs, linked, bck, cck, blocks: [(stored, payload offset, payload size)], consumed}."""
    assert struct.unpack_from("<I", frame, 0)[0] == 0x184D2204
    flg, bd = frame[4], frame[5]
    pos = 6 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0) + 1
    bck, cck = bool(flg & 0x10), bool(flg & 4)
    blocks = []
    while True:
        w = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        if w == 0: break
        n = w & 0x7FFFFFFF
        blocks.append((bool(w >> 31), pos, n))
        pos += n + (4 if bck else 0)
    return dict(flg=flg, bs=1 << (8 + 2 * ((bd >> 4) & 7)), linked=not flg & 0x20, bck=bck, cck=cck, blocks=blocks,
                content=struct.unpack_from("<Q", frame, 6)[0] if flg & 8 else None, consumed=pos + (4 if cck else 0))


class Verdict:
    def __init__(self, ok, out=b"", n_blocks=0, consumed=0, bad_block=None, why=""):
        self.ok, self.out, self.n_blocks, self.consumed, self.bad_block, self.why = ok, bytes(out), n_blocks, consumed, bad_block, why


def model_decode(frame: bytes, d: bytes) -> Verdict:
    """The dictionary model: every block through oracle.decompress_block with the dictionary's tail as history (and the output so
    far behind it when the blocks are linked)."""
    f = walk(frame)
    hist, out = tail(d), bytearray()
    for b, (stored, at, n) in enumerate(f["blocks"]):
        payload = frame[at:at + n]
        if f["bck"] and oracle.xxh32(payload) != struct.unpack_from("<I", frame, at + n)[0]:
            return Verdict(False, bad_block=b, why="block checksum")
        if stored: out += payload
        else:
            try: out += oracle.decompress_block(payload, f["bs"], hist + bytes(out) if f["linked"] else hist)
            except oracle.OracleError: return Verdict(False, bad_block=b, why="block")
    if f["content"] is not None and f["content"] != len(out): return Verdict(False, why="content size")
    if f["cck"] and oracle.xxh32(bytes(out)) != struct.unpack_from("<I", frame, f["consumed"] - 4)[0]: return Verdict(False, why="content checksum")
    return Verdict(True, out, len(f["blocks"]), f["consumed"])


def sequences(payload: bytes):
    """A compressed block's sequences as (literals, match length, offset); the last one has match length 0."""
    ip, n = 0, len(payload)
    while True:
        t = payload[ip]; ip += 1
        lit = t >> 4
        if lit == 15:
            while True:
                s = payload[ip]; ip += 1; lit += s
                if s != 255: break
        ip += lit
        if ip == n:
            yield lit, 0, 0
            return
        off = payload[ip] | payload[ip + 1] << 8; ip += 2
        ml = t & 15
        if ml == 15:
            while True:
                s = payload[ip]; ip += 1; ml += s
                if s != 255: break
        yield lit, ml + 4, off


# ---- the planted frames ----
def _lits(name: str, n: int) -> bytes:
    return rng_of("lit/" + name).integers(0, 256, n, dtype=np.uint8).tobytes()


def _sealed(name: str, d: bytes, linked: bool, blocks, bck=False, cck=False) -> bytes:
    """blocks: ('c', [sequences as (literals, mlen, off)]) or ('s', bytes).  Sealed with checksums where asked for (the content
    checksum is over what the model decodes the blocks to: a frame the model rejects is planted without one)."""
    fr = Frame(4, linked=linked, bck=bck, cck=False)
    for kind, x in blocks:
        if kind == "s": fr.stored(x)
        else: fr.raw_block(b"".join(lz4_seq(*s) for s in x), 0)
    if cck:
        v = model_decode(fr.bytes(), d)
        assert v.ok, name
        fr.cck, fr.out = True, bytearray(v.out)
    return fr.bytes()


def planted(dname: str) -> "list[tuple[str, str, bytes]]":
    """(name, mode, frame) for one dictionary.  D: the dictionary bytes that count."""
    key = ("planted", dname)
    if key in _cache: return _cache[key]
    d = dictionary(dname)
    D = min(len(d), KB64)
    L = lambda tag, n: _lits("%s/%s" % (dname, tag), n)
    end = lambda tag: (L(tag + "/end", 12), 0, 0)
    out = []

    def add(name, mode, blocks, **kw):
        out.append((name, mode, _sealed(name, d, mode == "linked", blocks, **kw)))

    for mode in MODES:
        add("first_match_op0", mode, [("c", [(b"", 8, min(D, 20)), end("a")])])
        if 10 + D <= 65535:
            add("off_exact", mode, [("c", [(L("b", 10), 6, 10 + D), end("b")])])             # the dictionary's first byte
        if 10 + D + 1 <= 65535:
            add("off_plus1", mode, [("c", [(L("c", 10), 6, 10 + D + 1), end("c")])])         # one byte in front of it: rejected
        if D == KB64:
            add("off65535_op0", mode, [("c", [(b"", 9, 65535), end("d")])])
        k = min(D, 5)
        add("cross", mode, [("c", [(L("e", 100), 40, 100 + k), end("e")])])                  # k bytes of dictionary, then the output's first bytes
        add("cross_cksums", mode, [("c", [(L("e", 100), 40, 100 + k), end("e")])], bck=True, cck=True)
        k2 = min(D, 2)
        add("cross_overlap", mode, [("c", [(L("f", 3), 40, 3 + k2), end("f")])])              # offset < mlen: through the seam into what the match writes
        add("cross_long", mode, [("c", [(L("g", 7), 3000, 7 + min(D, 1500)), end("g")])])     # both parts longer than a wave's round
        add("stored_between", mode, [("c", [(L("h", 20), 12, 20 + min(D, 9)), end("h")]), ("s", L("h/s", 50)),
                                     ("c", [(b"", 10, (0 if mode == "indep" else 20 + 12 + 12 + 50) + min(D, 16)), end("h2")])])
    # an independent frame whose second block opens with a match into the dictionary (its first block is a short one)
    add("second_block", "indep", [("c", [(L("i", 200), 0, 0)]), ("c", [(b"", 10, min(D, 16)), end("i")])])
    # a linked frame of short flushed blocks: the second block reaches through the first (100 bytes) into the dictionary
    k = min(D, 7)
    add("through_block1", "linked", [("c", [(L("j", 100), 0, 0)]), ("c", [(L("j2", 4), 20, 4 + 100 + k), end("j")])])
    if 4 + 100 + D + 1 <= 65535:
        add("through_block1_plus1", "linked", [("c", [(L("j", 100), 0, 0)]), ("c", [(L("j2", 4), 20, 4 + 100 + D + 1), end("j")])])
    # a linked frame whose third block lies past 64 KiB of output: the farthest offset there is (65 535) lands in the output, not in
    # the dictionary - with 64 KiB of output in front no 16-bit offset reaches a dictionary any more
    add("third_block_far", "linked", [("s", L("k", KB64)), ("s", L("k2", 100)), ("c", [(b"", 30, 65535), end("k")])])
    _cache[key] = out
    return out


# ---- the fixture ----
def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def check_sha(fx: dict):
    """Every regenerated dictionary, input and planted frame is the one the fixture was minted from - or fail loudly."""
    for dname in DICT_LEN:
        assert sha(dictionary(dname)) == fx["dicts"][dname]["sha256"], "dictionary %s is not the one the fixture was minted from" % dname
    for e in fx["natural"]:
        data = dict(natural(e["dict"]))[e["name"]]
        assert sha(data) == e["sha256"], "input %s/%s is not the one the fixture was minted from" % (e["dict"], e["name"])
    frames = {(dn, m, n): f for dn in DICT_LEN for n, m, f in planted(dn)}
    assert len(frames) == len(fx["planted"])
    for e in fx["planted"]:
        assert sha(frames[(e["dict"], e["mode"], e["name"])]) == e["sha256"], "planted %s/%s/%s differs from the minted one" % (e["dict"], e["mode"], e["name"])


def fixture_frames(fx: dict, dname: str, mode: str):
    """One dictionary's and one block mode's fixtures -> [(name, frame, expected output or None, liblz4's first bad block or None)]."""
    out = []
    nat = dict(natural(dname))
    for e in fx["natural"]:
        if e["dict"] == dname and e["mode"] == mode:
            out.append(("natural/" + e["name"], base64.b64decode(e["frame"]), nat[e["name"]], None))
    frames = {(m, n): f for n, m, f in planted(dname)}
    for e in fx["planted"]:
        if e["dict"] == dname and e["mode"] == mode:
            f = frames[(mode, e["name"])]
            exp = None
            if e["ok"]:
                exp = model_decode(f, dictionary(dname)).out                           # (held to liblz4's SHA-256 by the CPU test, and here)
                assert sha(exp) == e["out_sha256"], ("the model's bytes are not liblz4's", dname, mode, e["name"])
            out.append(("planted/" + e["name"], f, exp, e["bad_block"]))
    return out
