"""A plain model of this library's sequence index and in-band trailer (test helper, not a test module; numpy only).

The index (csrc/encode.cuh, "sequence index") is input to the decoder: it arrives beside the frame or inside the byte stream,
in the trailer (csrc/frame_dev.cuh, "the frame's trailer").  Its layout, in little-endian u32 words:
    IxHeader  magic 'LIX2', n_blocks, chunks_per_block, total_seqs, total_entries, stride 16, linked, 0
    IxBlock   per block: seq_base, nseq, entry_base, nentries          (stored block: nseq == nentries == 0)
    IxChunk   per block and chunk: ent_off, seq_off within the block   (ent_off bit 31: the block's final sequence follows
              this chunk's sequences - set on the block's last chunk with sequences)
    IxEntry   in_off (payload offset of the token), out_pos, seq_off (all within the block), nseq | block << 8
A chunk is pick_chunk_size(block size) = min(block size, 64 KiB) of the block's input (csrc/engine.hip); chunks_per_block is
block size / chunk.  The compressor's pass E2 writes an entry every 16 sequences OF A CHUNK, counting from the chunk's first
sequence; the block's final (literal-only) sequence rides on the last entry, which may then hold 17.

Which chunk a sequence belongs to is the tile of pass E1 that found its match.  That is not a function of the frame's bytes:
a match found at a position of chunk c may start before the chunk (extended backwards over literals) or run past its end.  So
`build()` places a sequence in the chunk where its match starts, and `violations()` checks what the decoders rely on plus the
rules every compressor-written index obeys:
  - the header names the frame's block count, this block size's chunking, stride 16, and totals equal to the block table's;
  - the block ranges tile [0, total_seqs) and [0, total_entries) in block order; stored blocks claim nothing, compressed
    blocks every sequence of their payload and at least one entry;
  - every entry names its own block, holds 1..16 sequences (17 only as the block's last, with the final sequence), starts where
    the one before ends (the first at sequence 0), and gives the true in_off and out_pos of its first sequence;
  - the chunks of a block start at (0, 0), never go backwards, each starts at an entry boundary; every entry of a chunk but its
    last holds 16 sequences; bit 31 is set on exactly the last chunk with sequences, and that chunk's entries end the block;
  - a sequence of chunk c has a match that overlaps input [c * chunk, (c + 1) * chunk) of its block.
"""
from __future__ import annotations

import struct

import numpy as np

IX_MAGIC = 0x3258494C
IX_STRIDE = 16
TR_MAGIC = 0x184D2A5E
TR_FOOT = 0x58495A4C
HDR_W, BLK_W, CHK_W, ENT_W = 8, 4, 2, 4                  # words per header / block / chunk / entry


def pick_chunk_size(bs: int) -> int:
    return min(bs, 64 << 10)


# ---------------------------------------------------------------------------------------------------------------------
class Parsed:
    """An LZ4 frame cut into blocks and sequences.  blocks[b] = dict(word_at, src_off, csize, stored, out_off, out_len,
    seqs): seqs is an (n, 5) int64 array (token's payload offset, output position, literals, match length, offset), the last
    row the block's final sequence (match length 0); None for stored blocks.  ValueError: a payload that does not parse."""

    def __init__(self, frame: bytes):
        f = memoryview(frame)
        assert struct.unpack_from("<I", f, 0)[0] == 0x184D2204, "not an LZ4 frame"
        flg, bd = f[4], f[5]
        self.linked = not (flg >> 5) & 1
        self.bck = bool((flg >> 4) & 1)
        self.cck = bool((flg >> 2) & 1)
        self.bsid = (bd >> 4) & 7
        self.bs = 1 << (8 + 2 * self.bsid)
        pos = 6 + (8 if (flg >> 3) & 1 else 0) + (4 if flg & 1 else 0) + 1
        self.blocks = []
        out = 0
        while True:
            word = struct.unpack_from("<I", f, pos)[0]
            if word == 0:
                pos += 4
                break
            csize, stored = word & 0x7FFFFFFF, bool(word >> 31)
            src = pos + 4
            if stored:
                seqs, n_out = None, csize
            else:
                try:
                    seqs, n_out = _parse_block(bytes(f[src:src + csize]))
                except IndexError:
                    raise ValueError("block %d: the payload ends inside a sequence" % len(self.blocks)) from None
            self.blocks.append(dict(word_at=pos, src_off=src, csize=csize, stored=stored, out_off=out, out_len=n_out, seqs=seqs))
            out += n_out
            pos = src + csize + (4 if self.bck else 0)
        if self.cck: pos += 4
        self.end = pos                                   # the frame's length (a trailer starts here)
        self.content = out


def _parse_block(p: bytes):
    """A compressed block's sequences (n, 5) and its output size; asserts on anything malformed."""
    pos, op, n = 0, 0, len(p)
    rows = []
    while True:
        at = pos
        tok = p[pos]; pos += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                v = p[pos]; pos += 1; lit += v
                if v != 255: break
        pos += lit
        if pos == n:
            rows.append((at, op, lit, 0, 0))
            op += lit
            break
        off = p[pos] | (p[pos + 1] << 8); pos += 2
        ml = tok & 15
        if ml == 15:
            while True:
                v = p[pos]; pos += 1; ml += v
                if v != 255: break
        ml += 4
        rows.append((at, op, lit, ml, off))
        op += lit + ml
        if pos >= n: raise ValueError("a match ends the payload")
    return np.array(rows, dtype=np.int64), op


# ---------------------------------------------------------------------------------------------------------------------
def fixed_words(n_blocks: int, cpb: int) -> int:
    return HDR_W + n_blocks * BLK_W + n_blocks * cpb * CHK_W


class View:
    """Named views into an index (a uint32 array, which it modifies in place)."""

    def __init__(self, ix: np.ndarray, n_blocks: int | None = None, cpb: int | None = None):
        self.w = ix
        self.n = int(ix[1]) if n_blocks is None else n_blocks
        self.cpb = int(ix[2]) if cpb is None else cpb
        self.blocks = ix[HDR_W:HDR_W + self.n * BLK_W].reshape(self.n, BLK_W)                  # seq_base, nseq, entry_base, nentries
        at = HDR_W + self.n * BLK_W
        self.chunks = ix[at:at + self.n * self.cpb * CHK_W].reshape(self.n, self.cpb, CHK_W)   # ent_off, seq_off
        e0 = fixed_words(self.n, self.cpb)
        self.entries = ix[e0:e0 + ((len(ix) - e0) // ENT_W) * ENT_W].reshape(-1, ENT_W)       # in_off, out_pos, seq_off, nseq | blk << 8


def chunk_of(seqs: np.ndarray, chunk: int) -> np.ndarray:
    """build()'s rule: the chunk where a sequence's match starts (the matches only: not the final sequence)."""
    return (seqs[:-1, 1] + seqs[:-1, 2]) // chunk


def build(frame: bytes, parsed: Parsed | None = None) -> np.ndarray:
    """A truthful index for any frame (uint32 array: header, tables, entries).  A compressed block without a match (the
    compressor never writes one) gets one entry holding its only sequence."""
    P = parsed or Parsed(frame)
    n, chunk = len(P.blocks), pick_chunk_size(P.bs)
    cpb = P.bs // chunk
    blocks = np.zeros((n, BLK_W), np.uint32)
    chunks = np.zeros((n, cpb, CHK_W), np.uint32)
    ents = []
    sb = eb = 0
    for b, B in enumerate(P.blocks):
        blocks[b, 0], blocks[b, 2] = sb, eb
        if B["stored"]: continue
        S = B["seqs"]
        nm = len(S) - 1                                   # sequences with a match
        cid = chunk_of(S, chunk)
        nent = 0
        if nm == 0:
            chunks[b, 1:, 0] = 1
            chunks[b, 0, 0] = 0x80000000
            ents.append((S[0, 0], S[0, 1], 0, 1 | (b << 8)))
            nent = 1
        else:
            last = int(cid[-1])
            i = 0
            for c in range(cpb):
                chunks[b, c] = (nent | (0x80000000 if c == last else 0), i)
                j = i
                while j < nm and cid[j] == c: j += 1
                for k in range(i, j, IX_STRIDE):
                    ns = min(IX_STRIDE, j - k) + (1 if c == last and k + IX_STRIDE >= j else 0)
                    ents.append((S[k, 0], S[k, 1], k, ns | (b << 8)))
                    nent += 1
                i = j
        blocks[b, 1], blocks[b, 3] = len(S), nent
        sb += len(S); eb += nent
    hdr = np.array([IX_MAGIC, n, cpb, sb, eb, IX_STRIDE, 1 if P.linked else 0, 0], np.uint32)
    return np.concatenate([hdr, blocks.ravel(), chunks.ravel(), np.array(ents, np.uint32).reshape(-1)])


def index_bytes(ix: np.ndarray) -> bytes:
    return np.ascontiguousarray(ix, dtype="<u4").tobytes()


def violations(frame: bytes, ix: np.ndarray, parsed: Parsed | None = None) -> list[str]:
    """What in `ix` disagrees with the frame (see the module docstring); [] for a truthful index."""
    P = parsed or Parsed(frame)
    ix = np.asarray(ix, dtype=np.uint32)
    n, chunk = len(P.blocks), pick_chunk_size(P.bs)
    cpb = P.bs // chunk
    bad = []
    if len(ix) < HDR_W: return ["shorter than its header"]
    h = [int(x) for x in ix[:HDR_W]]
    if h[0] != IX_MAGIC: bad.append("magic")
    if h[1] != n: bad.append("header n_blocks %d, frame %d" % (h[1], n))
    if h[2] != cpb: bad.append("header chunks_per_block %d, want %d" % (h[2], cpb))
    if h[5] != IX_STRIDE: bad.append("stride %d" % h[5])
    if h[6] != (1 if P.linked else 0) or h[7] != 0: bad.append("header pad words")
    if bad: return bad
    if len(ix) < fixed_words(n, cpb) + h[4] * ENT_W: return bad + ["shorter than its tables and %d entries" % h[4]]
    V = View(ix, n, cpb)
    E = V.entries[:h[4]].astype(np.int64)
    sb = eb = 0
    for b, B in enumerate(P.blocks):
        base, ns, ebase, ne = (int(x) for x in V.blocks[b])
        if base != sb or ebase != eb: bad.append("block %d: base (%d, %d), want (%d, %d)" % (b, base, ebase, sb, eb))
        sb, eb = base + ns, ebase + ne
        if B["stored"]:
            if ns or ne: bad.append("stored block %d claims %d sequences, %d entries" % (b, ns, ne))
            continue
        S = B["seqs"]
        if ns != len(S) or ne == 0:
            bad.append("block %d: %d sequences / %d entries, payload has %d sequences" % (b, ns, ne, len(S)))
            continue
        if ebase + ne > h[4]:
            bad.append("block %d: entries beyond the total" % b)
            continue
        e = E[ebase:ebase + ne]
        cnt = e[:, 3] & 0xFF
        if np.any(e[:, 3] >> 8 != b): bad.append("block %d: an entry names another block" % b)
        if np.any(cnt == 0) or np.any(cnt[:-1] > IX_STRIDE) or cnt[-1] > IX_STRIDE + 1: bad.append("block %d: entry sequence counts" % b)
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        if not np.array_equal(e[:, 2], starts) or int(cnt.sum()) != ns:
            bad.append("block %d: entries' seq_off do not tile its sequences" % b)
            continue
        if not np.array_equal(e[:, 0], S[starts, 0]): bad.append("block %d: entry in_off" % b)
        if not np.array_equal(e[:, 1], S[starts, 1]): bad.append("block %d: entry out_pos" % b)
        # chunks
        C = V.chunks[b].astype(np.int64)
        eo, so, fin = C[:, 0] & 0x7FFFFFFF, C[:, 1], C[:, 0] >> 31
        if eo[0] != 0 or so[0] != 0 or np.any(np.diff(eo) < 0) or np.any(np.diff(so) < 0):
            bad.append("block %d: chunk table does not start at 0 or goes backwards" % b)
            continue
        if np.any(eo > ne) or np.any(so > ns): bad.append("block %d: chunk beyond the block" % b); continue
        ent_first = {int(s): k for k, s in enumerate(starts)}
        nonempty = [c for c in range(cpb) if (eo[c + 1] if c + 1 < cpb else ne) > eo[c]]
        if not nonempty or int(fin.sum()) != 1 or fin[nonempty[-1]] != 1:
            bad.append("block %d: final-sequence mark" % b)
            continue
        last = nonempty[-1]
        nm = len(S) - 1
        for c in range(cpb):
            e_hi = eo[c + 1] if c + 1 < cpb else ne
            s_hi = so[c + 1] if c + 1 < cpb else nm
            if e_hi == eo[c]:
                if s_hi != so[c]: bad.append("block %d chunk %d: sequences without entries" % (b, c))
                continue
            if c > last: bad.append("block %d chunk %d: entries behind the marked chunk" % (b, c)); continue
            if ent_first.get(int(so[c])) != eo[c]: bad.append("block %d chunk %d: does not start at its entry" % (b, c)); continue
            mine = cnt[eo[c]:e_hi]
            if np.any(mine[:-1] != IX_STRIDE): bad.append("block %d chunk %d: an inner entry short of 16" % (b, c))
            if int(mine.sum()) - (1 if c == last else 0) != s_hi - so[c]: bad.append("block %d chunk %d: sequence count" % (b, c))
            if nm:
                m = S[so[c]:min(s_hi, nm)]
                ms, me = m[:, 1] + m[:, 2], m[:, 1] + m[:, 2] + m[:, 3]
                if np.any(ms >= (c + 1) * chunk) or np.any(me <= c * chunk): bad.append("block %d chunk %d: a match outside the chunk" % (b, c))
    if sb != h[3] or eb != h[4]: bad.append("totals (%d, %d), header (%d, %d)" % (sb, eb, h[3], h[4]))
    return bad


def truthful(frame: bytes, ix: np.ndarray, parsed: Parsed | None = None) -> bool:
    return not violations(frame, ix, parsed)


def usable_by_decoder(ix: np.ndarray) -> bool:
    return len(ix) >= HDR_W and int(ix[0]) == IX_MAGIC and int(ix[5]) == IX_STRIDE


# ---------------------------------------------------------------------------------------------------------------------
# The trailer: frame | 5E 2A 4D 18 | u32 size | zeros to 16 | u64 size-word positions (n_blocks, to even) | index | footer
def _round16(x: int) -> int:
    return (x + 15) & ~15


def trailer(frame: bytes, ix: np.ndarray | None, parsed: Parsed | None = None) -> bytes:
    """The trailer k_trailer_plan / k_trailer_copy put behind `frame` (which starts the stream at offset 0); `ix` None: the
    block list alone.  The index is padded with zeros to 16 bytes (the compressor copies whatever its buffer holds there)."""
    P = parsed or Parsed(frame)
    F, n = len(frame), len(P.blocks)
    list_at = _round16(F + 8)
    n_list = (n + 1) & ~1
    lst = [B["word_at"] for B in P.blocks] + [0] * (n_list - n)
    ixb = b"" if ix is None else index_bytes(ix)
    ixb += bytes(_round16(len(ixb)) - len(ixb))
    total = list_at + 8 * n_list + len(ixb) + 32 - F
    seqs, ents = (0, 0) if ix is None else (int(ix[3]), int(ix[4]))
    return (struct.pack("<II", TR_MAGIC, total - 8) + bytes(list_at - F - 8) + struct.pack("<%dQ" % n_list, *lst) + ixb +
            struct.pack("<IIIIIIQ", seqs, ents, 0, 0, TR_FOOT, n, total))


def read_trailer(stream: bytes, frame_len: int):
    """(list of size-word positions, index words or None, footer dict) of the trailer behind stream[:frame_len]."""
    t = stream[frame_len:]
    magic, size = struct.unpack_from("<II", t, 0)
    assert magic == TR_MAGIC and size == len(t) - 8
    seqs, ents, p0, p1, fm, n, total = struct.unpack_from("<IIIIIIQ", t, len(t) - 32)
    assert fm == TR_FOOT and total == len(t) and p0 == p1 == 0
    list_at = _round16(frame_len + 8) - frame_len
    n_list = (n + 1) & ~1
    lst = list(struct.unpack_from("<%dQ" % n_list, t, list_at))
    ix_at = list_at + 8 * n_list
    ixb = t[ix_at:len(t) - 32]
    ix = np.frombuffer(ixb, dtype="<u4").astype(np.uint32) if ixb else None
    return lst, ix, dict(total_seqs=seqs, total_entries=ents, n_blocks=n, total=total)


def splice(stream_frame: bytes, tr: bytes) -> bytes:
    return stream_frame + tr


# ---------------------------------------------------------------------------------------------------------------------
# Forgeries: each breaks exactly one thing and keeps everything else consistent.  Named; rebuilt from the name alone.
def _pick_k(P: Parsed) -> int:
    """The block forgeries aim at: the middle compressed block with a compressed block in front of it."""
    comp = [b for b, B in enumerate(P.blocks) if not B["stored"] and b > 0 and not P.blocks[b - 1]["stored"]]
    assert comp, "the frame needs two compressed blocks in a row"
    return comp[len(comp) // 2]


def forgery_names(frame: bytes, parsed: Parsed | None = None) -> list[str]:
    P = parsed or Parsed(frame)
    has_stored = any(B["stored"] for B in P.blocks)
    names = []
    for D in ("1", "64", "2^20", "0x7FFFFFFF", "2^32-base-1"):
        names.append("table/seq_suffix_shift/" + D)
        names.append("table/entry_suffix_shift/" + D)
    names += ["table/seq_overlap_prev", "table/entry_overlap_prev", "table/seq_move_one", "table/entry_move_one",
              "table/compressed_claims_none", "table/last_seq_end-1", "table/last_seq_end+1", "table/last_entry_end-1",
              "table/last_entry_end+1"]
    if has_stored: names.append("table/stored_claims_seqs")
    names += ["header/n_blocks-1", "header/n_blocks+1", "header/chunks_per_block-1", "header/chunks_per_block+1",
              "header/stride15", "header/stride17", "header/total_seqs_at_cap", "header/total_seqs_above_cap",
              "header/total_entries_at_bound", "header/total_entries_above_bound"]
    names += ["entry/in_off-1", "entry/in_off+1", "entry/out_pos+1", "entry/out_pos_block_shift", "entry/seq_off+1",
              "entry/nseq0", "entry/nseq17", "entry/nseq255", "entry/wrong_block", "entry/first_nonzero"]
    names += ["footer/counts_smaller", "footer/counts_larger", "footer/n_blocks-1", "footer/n_blocks+1", "footer/total_inside_index"]
    return names


def _D(spec: str, base: int) -> int:
    return {"1": 1, "64": 64, "2^20": 1 << 20, "0x7FFFFFFF": 0x7FFFFFFF, "2^32-base-1": (1 << 32) - base - 1}[spec]


def forge(frame: bytes, ix: np.ndarray, name: str, parsed: Parsed | None = None) -> np.ndarray:
    """The index forgery `name` of `ix` (a new array, same length).  footer/* forgeries leave the index as it is: see
    forge_trailer()."""
    P = parsed or Parsed(frame)
    f = np.array(ix, dtype=np.uint32, copy=True)
    V = View(f)
    n = V.n
    k = _pick_k(P)
    fam, what = name.split("/", 1)
    M = 0xFFFFFFFF
    if fam == "table":
        bl = V.blocks
        if what.startswith("seq_suffix_shift/") or what.startswith("entry_suffix_shift/"):
            col = 0 if what.startswith("seq") else 2
            D = _D(what.split("/")[1], int(bl[k, col]))
            bl[k:, col] = (bl[k:, col].astype(np.uint64) + D) & M              # only the link k-1 -> k breaks (and the last block's end)
        elif what in ("seq_overlap_prev", "entry_overlap_prev"):
            col = 0 if what.startswith("seq") else 2                             # k starts inside k-1; k's own link to k+1 holds
            s = 1 if bl[k - 1, col + 1] > 1 else 0
            bl[k, col] -= s; bl[k, col + 1] += s
        elif what in ("seq_move_one", "entry_move_one"):
            col = 0 if what.startswith("seq") else 2                             # one sequence / entry from k-1 to k: totals and links hold
            bl[k - 1, col + 1] -= 1; bl[k, col] -= 1; bl[k, col + 1] += 1
        elif what == "compressed_claims_none":                                  # block k's sequences and entries go to k-1
            bl[k - 1, 1] += bl[k, 1]; bl[k - 1, 3] += bl[k, 3]
            bl[k, 0] = bl[k - 1, 0] + bl[k - 1, 1]; bl[k, 2] = bl[k - 1, 2] + bl[k - 1, 3]; bl[k, 1] = 0; bl[k, 3] = 0
        elif what == "stored_claims_seqs":                                      # a stored block takes one sequence from the block in front
            s = next(b for b, B in enumerate(P.blocks) if B["stored"])
            p = s - 1 if s > 0 else s + 1
            if p < s: bl[p, 1] -= 1; bl[s, 0] -= 1; bl[s, 1] += 1
            else: bl[s, 1] += 1; bl[p, 0] += 1; bl[p, 1] -= 1
        elif what.startswith("last_seq_end") or what.startswith("last_entry_end"):
            col = 1 if "seq" in what else 3
            d = -1 if what.endswith("-1") else 1
            last = max(b for b, B in enumerate(P.blocks) if not B["stored"])
            bl[last, col] = (int(bl[last, col]) + d) & M                         # the last range ends short of or past the header's total
        else: raise KeyError(name)
    elif fam == "header":
        if what == "n_blocks-1": f[1] -= 1
        elif what == "n_blocks+1": f[1] += 1
        elif what == "chunks_per_block-1": f[2] -= 1
        elif what == "chunks_per_block+1": f[2] += 1
        elif what == "stride15": f[5] = 15
        elif what == "stride17": f[5] = 17
        elif what == "total_seqs_at_cap": f[3] = min(int(f[4]) * (IX_STRIDE + 1), M)            # the most the entries could hold
        elif what == "total_seqs_above_cap": f[3] = min(int(f[4]) * (IX_STRIDE + 1) + 1, M)
        elif what.startswith("total_entries"):
            bound = (len(f) - fixed_words(n, V.cpb)) // ENT_W                   # the most the buffer holds
            f[4] = bound if what.endswith("at_bound") else bound + 1
        else: raise KeyError(name)
    elif fam == "entry":
        E = V.entries
        eb, ne = int(V.blocks[k, 2]), int(V.blocks[k, 3])
        mid = eb + max(1, ne // 2) if ne > 1 else eb                              # (not the first entry: first_nonzero is that one)
        if what == "in_off-1": E[mid, 0] -= 1
        elif what == "in_off+1": E[mid, 0] += 1
        elif what == "out_pos+1": E[mid, 1] += 1
        elif what == "out_pos_block_shift": E[eb:eb + ne, 1] += P.bs
        elif what == "seq_off+1": E[mid, 2] += 1
        elif what in ("nseq0", "nseq17", "nseq255"):
            E[mid, 3] = (E[mid, 3] & ~np.uint32(0xFF)) | {"nseq0": 0, "nseq17": 17, "nseq255": 255}[what]
        elif what == "wrong_block": E[mid, 3] = (E[mid, 3] & 0xFF) | (((k - 1) & 0xFFFFFF) << 8)
        elif what == "first_nonzero":                                            # the block's first entry starts at its second sequence
            E[eb, 0] = P.blocks[k]["seqs"][1, 0]; E[eb, 1] = P.blocks[k]["seqs"][1, 1]; E[eb, 2] = 1
        else: raise KeyError(name)
    elif fam == "footer":
        pass
    else: raise KeyError(name)
    return f


def forge_trailer(frame: bytes, ix: np.ndarray, name: str, parsed: Parsed | None = None) -> bytes:
    """frame + a trailer carrying forgery `name`: an index forgery, or a footer that lies while the rest holds."""
    P = parsed or Parsed(frame)
    fam, what = name.split("/", 1)
    if fam != "footer": return frame + trailer(frame, forge(frame, ix, name, P), P)
    tr = bytearray(trailer(frame, ix, P))
    seqs, ents, p0, p1, fm, nb, total = struct.unpack_from("<IIIIIIQ", tr, len(tr) - 32)
    if what == "counts_smaller": seqs, ents = seqs - 1, ents - 1
    elif what == "counts_larger": seqs, ents = seqs + 1, ents + 1
    elif what == "n_blocks-1": nb -= 1
    elif what == "n_blocks+1": nb += 1
    elif what == "total_inside_index":                                            # the trailer claims to start inside the index
        total = 32 + 16 * max(1, int(ix[4]) // 2)
    else: raise KeyError(name)
    struct.pack_into("<IIIIIIQ", tr, len(tr) - 32, seqs, ents, p0, p1, fm, nb, total)
    return frame + bytes(tr)


def forgeries(frame: bytes, ix: np.ndarray, parsed: Parsed | None = None) -> list[tuple[str, np.ndarray]]:
    """[(name, forged index)] for every index forgery (footer forgeries: forge_trailer)."""
    P = parsed or Parsed(frame)
    return [(nm, forge(frame, ix, nm, P)) for nm in forgery_names(frame, P) if not nm.startswith("footer/")]


def trailer_violations(stream: bytes, frame_len: int) -> list[str]:
    """What in the trailer behind stream[:frame_len] disagrees with the frame: the list, the footer, the index (if any)."""
    frame = stream[:frame_len]
    P = Parsed(frame)
    try:
        lst, ix, ft = read_trailer(stream, frame_len)
    except (AssertionError, struct.error) as e:
        return ["trailer layout: %s" % e]
    bad = []
    n = len(P.blocks)
    if ft["n_blocks"] != n: bad.append("footer n_blocks %d, frame %d" % (ft["n_blocks"], n))
    if lst[:n] != [B["word_at"] for B in P.blocks] or any(lst[n:]): bad.append("block list")
    if ix is None:
        if ft["total_seqs"] or ft["total_entries"]: bad.append("footer counts without an index")
        return bad
    if (ft["total_seqs"], ft["total_entries"]) != (int(ix[3]), int(ix[4])): bad.append("footer counts differ from the header's")
    if len(ix) * 4 != _round16(fixed_words(int(ix[1]), int(ix[2])) * 4 + int(ix[4]) * 16): bad.append("index region size")
    return bad + violations(frame, ix, P)
