"""What the LZ4 block and frame formats require of a WRITER, checked on a finished frame (test helper, not a test module; numpy only).

A decoder - liblz4's, which oracle/orc_lz4block.c restates, and this library's - is more generous than the format: it does not ask that
the last match start 12 bytes before the block's end, and it bounds the end-of-block rules by the frame's maxBlockSize, not by the
block's own length, so a short last block is not checked at all.  A frame can therefore round-trip through every decoder here and
still be refused by a strict one.  `audit(frame, data)` holds a frame to the writer's side of lz4_Block_format.md ("End of block
restrictions") and lz4_Frame_format.md, independently of the library: it is built on lz4_index.Parsed alone.

Each violation is a string "rule: detail"; `rules(violations)` gives the set of rule names.  The rules:

  frame    header         FLG / BD name the version, block size, block mode and checksum flags of the preferences (`want`, if given)
           endmark        the block list ends in a zero size word (and a payload parses to its end)
           block-checksum, content-checksum      equal oracle.xxh32 of the payload as stored / of `data`
  blocks   size-word      a block's size word is at most maxBlockSize
           not-smaller    a compressed block's payload is strictly smaller than what it decodes to (otherwise the writer stores it)
           block-length   every block but the last decodes to exactly maxBlockSize, none to nothing (a stored block's size IS its
                          length, so this is also the rule that a stored block's size equals its length)
           content-length the block lengths sum to len(data)
  compressed block of decoded length blen
           last-literals  the final sequence has at least 5 literals - unless blen < 5, where it is the whole block.  The final
                          sequence is literals only by the grammar, and it begins where the last match ends: so this is also the rule
                          that every match ends at or before blen - 5 (an earlier match ends before the last one does).
           short-block-match   no match if blen < 13
           match-start    every match starts at or before blen - 12
           offset-range   every offset is in 1..65535 (only 0 can be written wrong: the field has 16 bits)
           offset-reach   every offset is at most the match's position in the block plus what lies in front of the block: the
                          dictionary's dict_len bytes (the batch calls' shared dictionary; 0 without one), in a linked frame
                          min(bytes in front of the block + dict_len, 65536)
A match length below 4 cannot be written (the token holds length - 4), so there is no rule for it.
"""
from __future__ import annotations

import struct

import numpy as np

from lz4_index import Parsed


def _xxh32(b) -> int:
    import oracle
    return oracle.xxh32(bytes(b))


def rules(violations) -> set:
    return {v.split(":", 1)[0] for v in violations}


def audit(frame: bytes, data: bytes, want: dict | None = None, parsed: Parsed | None = None, dict_len: int = 0) -> list[str]:
    """The writer rules `frame` breaks as a frame of `data`; [] for a frame a strict decoder accepts.  `want`: the preferences the
    header must name - dict(bsid, linked, bck, cck), any subset.  `parsed`: Parsed(frame), if the caller has it.  `dict_len`: the
    bytes of the dictionary the frame was written with that count (at most 65536): they lie in front of every block of an
    independent frame and in front of a linked frame's first byte."""
    bad = []
    if len(frame) < 7 or struct.unpack_from("<I", frame, 0)[0] != 0x184D2204: return ["header: no LZ4 frame magic"]
    flg, bd = frame[4], frame[5]
    if flg >> 6 != 1 or flg & 2 or bd & 0x8F or not 4 <= (bd >> 4) & 7 <= 7: bad.append("header: FLG %02x BD %02x: version, reserved bits or block size" % (flg, bd))
    hlen = 6 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if frame[hlen] != (_xxh32(frame[4:hlen]) >> 8) & 0xFF: bad.append("header: header checksum")
    if bad: return bad
    try:
        P = parsed or Parsed(frame)
    except (struct.error, ValueError, IndexError) as e:
        return ["endmark: the block list does not parse to an EndMark (%s)" % e]
    if want:
        got = dict(bsid=P.bsid, linked=P.linked, bck=P.bck, cck=P.cck)
        for k, v in want.items():
            if got[k] != v: bad.append("header: %s is %r, the preferences say %r" % (k, got[k], v))
    if P.end > len(frame): bad.append("endmark: the frame ends inside its checksum")
    n = len(data)
    for b, B in enumerate(P.blocks):
        blen, last = B["out_len"], b + 1 == len(P.blocks)
        if B["csize"] > P.bs: bad.append("size-word: block %d says %d, maxBlockSize is %d" % (b, B["csize"], P.bs))
        if blen == 0 or blen > P.bs or (not last and blen != P.bs):
            bad.append("block-length: block %d of %d decodes to %d bytes, maxBlockSize is %d" % (b, len(P.blocks), blen, P.bs))
        if P.bck:
            stored = struct.unpack_from("<I", frame, B["src_off"] + B["csize"])[0]
            if stored != _xxh32(frame[B["src_off"]:B["src_off"] + B["csize"]]): bad.append("block-checksum: block %d" % b)
        if B["stored"]: continue
        if B["csize"] >= blen: bad.append("not-smaller: block %d: a payload of %d bytes for %d" % (b, B["csize"], blen))
        S = B["seqs"]
        fin = int(S[-1, 2])
        if (fin < 5 and blen >= 5) or (blen < 5 and len(S) > 1):
            bad.append("last-literals: block %d of %d bytes ends in %d literals: its last match ends at blen - %d" % (b, blen, fin, fin))
        M = S[:-1]
        if len(M) == 0: continue
        start = M[:, 1] + M[:, 2]
        if blen < 13: bad.append("short-block-match: block %d of %d bytes has %d" % (b, blen, len(M)))
        elif np.any(start > blen - 12):
            k = int(np.argmax(start > blen - 12))
            bad.append("match-start: block %d of %d bytes: sequence %d's match starts at blen - %d" % (b, blen, k, blen - int(start[k])))
        if np.any(M[:, 4] < 1) or np.any(M[:, 4] > 65535):
            bad.append("offset-range: block %d: offset %d" % (b, int(M[np.argmax((M[:, 4] < 1) | (M[:, 4] > 65535)), 4])))
        reach = start + (min(B["out_off"] + dict_len, 65536) if P.linked else dict_len)
        if np.any(M[:, 4] > reach):
            k = int(np.argmax(M[:, 4] > reach))
            bad.append("offset-reach: block %d: sequence %d at %d has offset %d, reach %d" % (b, k, int(start[k]), int(M[k, 4]), int(reach[k])))
    if P.content != n: bad.append("content-length: the blocks decode to %d bytes, the input has %d" % (P.content, n))
    if P.cck and P.end <= len(frame) and struct.unpack_from("<I", frame, P.end - 4)[0] != _xxh32(data): bad.append("content-checksum")
    return bad


def matches(frame: bytes, parsed: Parsed | None = None) -> np.ndarray:
    """The frame's matches as (position in the content, length, offset, literals in front) rows, neighbours merged: a match that
    begins where the one before ends, at the same offset, is its continuation (a repeat cut at a 64 KiB chunk seam, or at a length
    cap).  The `literals in front` of a block's first match count from the block's start."""
    P = parsed or Parsed(frame)
    rows = []
    for B in P.blocks:
        if B["stored"]: continue
        for at, op, lit, ml, off in B["seqs"][:-1].tolist():
            pos = B["out_off"] + op + lit
            if lit == 0 and rows and rows[-1][2] == off and rows[-1][0] + rows[-1][1] == pos and pos > B["out_off"]:
                rows[-1][1] += ml
            else:
                rows.append([pos, ml, off, lit])
    return np.array(rows, dtype=np.int64).reshape(-1, 4)
