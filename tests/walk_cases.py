"""The case list of the block-table walks (test helper, not a test module): tests/test_gpu_walks.py runs it on the GPU,
tests/test_walk_cases_cpu.py holds the same list to the oracle and to a plain walk without one.

A frame that comes without a block table gets one from a walk over its size words (engine.hip: decode_plan): the serial walk, or
one of three that GUESS a list of positions - the parallel walk (blocks <= 256 KiB, frame_cap >= 1 MiB), the seeded walk (bigger
blocks, frame_cap >= 192 block sizes), the trailer's list.  A guessed list is accepted only if it is the chain the size words
form, from the header to the first EndMark; otherwise the serial walk runs behind.  The cases here are built against the seams
of the three: chunk, group and stride boundaries, the slot and list limits, seed windows, decoy chains, lying trailers, and
malformed frames of a size at which a guessing walk is planned.

Every case is rebuilt from its name alone (case(name)): numpy's PCG64 seeded with the name's CRC32 draws what is drawn.  A case is
a buffer of `cap` payload-like bytes (1..0x7F: no word made of them has a top byte of 0x00 or 0x80, so none can start a chain) and
a short list of operations that plant everything else - header, size words, checksums (taken once everything else is planted),
decoys, zeros, and "late" bytes that damage a checksum.  Frames are made of STORED
blocks, so the expected output is a list of ranges of the buffer itself, and a frame of any size costs milliseconds: the seeded
cases are made on the device from the same operations (test_gpu_walks.py), and checked here at a few blocks (big=False).

The frame layout is restated here on purpose (no helper of the library, none of the other tests' walks)."""
import struct
import zlib

import numpy as np

MAGIC, SKIP0, TR_MAGIC, TR_FOOT = 0x184D2204, 0x184D2A50, 0x184D2A5E, 0x58495A4C
STORED, NONE = 0x80000000, 0xFFFFFFFF
# frame_dev.cuh / engine.hip (decode_plan): the walks' constants, restated
WK_CHUNK, WK_SLOTS, WK_HOPS = 65536, 30, 3
WK_GROUP, WK_STRIDE, WK_TAIL = 16, 4096, 20
WK_SEEDS, WK_SEED_HOPS, WK_SEED_PIECE, WK_SEED_LIST, WK_LANE_CAP = 64, 4, 131072, 2048, 192
PAR_MAX_BS, PAR_MIN_CAP, SEED_BLOCKS, LIST_SLACK = 256 << 10, 1 << 20, 192, 1024
SMALL_SEED_BLOCKS = 3                  # the seeded recipes at big=False: this many block sizes stand in for the 192

ST = dict(ok=0, generic=1, maxblock=2, version=6, blockck=7, reserved=8, dstsmall=11, incomplete=12, frametype=13, framesize=14, headerck=17,
          contentck=18)


def le32(v): return struct.pack("<I", v & 0xFFFFFFFF)
def le64(v): return struct.pack("<Q", v & 0xFFFFFFFFFFFFFFFF)
def u32(b): return struct.unpack("<I", bytes(b))[0]
def bs_of(bsid): return 1 << (8 + 2 * bsid)


def xxh32(b) -> int:
    import oracle                      # (the CPU restatement the whole suite is pinned to; not the library under test)
    return oracle.xxh32(bytes(b))


class Case:
    """name, kind ("parallel" | "seeded" | "trailer"), cap (the frame_cap to pass; the buffer is exactly that long), room (the
    output capacity), ops (what is planted, in order), words / lens (the first frame's size-word positions and payload lengths,
    as far as the frame is sound), segs ((position, length) of the expected output in the buffer), decoys (planted positions that
    are candidates by the rule but no block starts), expect, planned ("parallel" | "trailer" | "serial": the path bit - the seeded
    walk reports LZ4F_MI355X_PATH_PARALLEL_WALK too), seams."""

    def __init__(self, name, kind, bsid, bck=0, cck=0, csize=0):
        self.name, self.kind, self.bsid, self.bs, self.bck, self.cck, self.csize = name, kind, bsid, bs_of(bsid), bck, cck, csize
        self.ops, self.words, self.lens, self.segs, self.decoys, self.seams = [], [], [], [], [], []
        self.cap = self.room = 0
        self.big = False
        self.bare = None               # trailer cases: the name of the case whose record and bytes this one must give
        self.hsize = 7 + (8 if csize else 0)
        self.rng = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))

    # ---- planting
    def put(self, pos, b): self.ops.append(("bytes", pos, bytes(b)))
    def fill(self, pos, n, v): self.ops.append(("fill", pos, n, v))
    def rand(self, pos, n): self.ops.append(("bytes", pos, self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    def xxh(self, pos, segs): self.ops.append(("xxh", pos, list(segs)))

    def header(self, at=0, content=0, wrong_hc=False):
        flg = 0x40 | 0x20 | (self.bck << 4) | ((1 if self.csize else 0) << 3) | (self.cck << 2)
        d = bytes([flg, self.bsid << 4]) + (le64(content) if self.csize else b"")
        hc = (xxh32(d) >> 8) & 0xFF
        self.put(at, le32(MAGIC) + d + bytes([hc ^ (0x5A if wrong_hc else 0)]))
        return at + 4 + len(d) + 1

    def chain(self, at, lens, first=True, endmark=True, tail=True, words=None):
        """Stored blocks of `lens` bytes from `at` on, the EndMark, the content checksum -> the position behind.  words: {block:
        size word} to plant instead of the right one (the walk ends there: what follows is laid out as if it were right)."""
        pos, segs, sound = at, [], True
        for i, n in enumerate(lens):
            w = STORED | n
            if words and i in words:
                w, sound = words[i], False
            self.put(pos, le32(w))
            if first and sound:
                self.words.append(pos); self.lens.append(n)
            segs.append((pos + 4, n))
            if self.bck:
                self.xxh(pos + 4 + n, [(pos + 4, n)])
            pos += 4 + n + 4 * self.bck
        if first:
            self.segs = segs
        if endmark:
            self.put(pos, le32(0)); pos += 4
            if tail and self.cck:
                self.xxh(pos, segs); pos += 4
        return pos

    def frame(self, lens, **kw):
        at = self.header(content=sum(lens))
        assert at == self.hsize
        return self.chain(at, lens, **kw)

    def done(self, cap, expect, planned, seams, room=None):
        self.cap, self.expect, self.planned = cap, expect, planned
        self.room = len(self.segs) * self.bs if room is None else room
        self.seams = list(seams)
        assert all(op[1] >= 0 and op[1] + (op[2] if op[0] == "fill" else len(op[2]) if op[0] in ("bytes", "late") else 4) <= cap for op in self.ops), self.name
        if planned == "parallel": assert self.bs <= PAR_MAX_BS and cap >= PAR_MIN_CAP, (self.name, cap)
        return self

    @property
    def content_len(self): return sum(n for _, n in self.segs)


def materialize(c: Case) -> np.ndarray:
    """The case's buffer (numpy, host)."""
    bg = np.random.Generator(np.random.PCG64(zlib.crc32(c.name.encode())).jumped(1))
    a = bg.integers(1, 0x80, c.cap, dtype=np.uint8)
    for kinds in (("bytes", "fill"), ("xxh",), ("late",)):      # what is planted; then the checksums over it; then what damages one
        for op in c.ops:
            if op[0] not in kinds: continue
            if op[0] in ("bytes", "late"): a[op[1]:op[1] + len(op[2])] = np.frombuffer(op[2], dtype=np.uint8)
            elif op[0] == "fill": a[op[1]:op[1] + op[2]] = op[3]
            else: a[op[1]:op[1] + 4] = np.frombuffer(le32(xxh32(b"".join(a[p:p + n].tobytes() for p, n in op[2]))), dtype=np.uint8)
    return a


def content_of(c: Case, a) -> bytes:
    return b"".join(bytes(a[p:p + n]) for p, n in c.segs)


# ---- the plain walk: what the record of a frame decode must be (lz4f_mi355x.h: lz4f_mi355x_result) ---------------------------
def model_record(read, cap: int, room: int, checks: bool = True) -> dict:
    """read(pos, n) -> bytes of the buffer.  The record lz4f_mi355x_dev_decompressFrame must write for the first frame in
    buffer[0:cap] decoded into `room` bytes, for frames of stored blocks: status, size, consumed, n_blocks, first_bad_block,
    flags & 0x1FF.  A frame that fails before its blocks are decoded has size, consumed and n_blocks 0; one whose walk is sound
    and whose block or content fails keeps the walk's n_blocks and consumed, and `size` is the header's content size (0 without).
    "host": the call itself returns the error (a descriptor the host refuses), no record is written."""
    r = dict(status=0, size=0, consumed=0, n_blocks=0, first_bad_block=NONE, flags=0, host=False)
    def fail(st, host=False):
        r.update(status=ST[st], host=host); return r
    if cap < 7: return fail("incomplete", True)
    magic = u32(read(0, 4))
    if magic & 0xFFFFFFF0 == SKIP0:
        if cap < 8: return fail("incomplete")
        n = 8 + u32(read(4, 4))
        if cap < n: return fail("incomplete")
        r.update(consumed=n, flags=0x100); return r
    if magic != MAGIC: return fail("frametype")
    flg, bd = read(4, 1)[0], read(5, 1)[0]
    if flg & 2: return fail("reserved", True)
    if flg >> 6 != 1: return fail("version", True)
    hsize = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if cap < hsize: return fail("incomplete", True)
    if bd & 0x80: return fail("reserved", True)
    if (bd >> 4) & 7 < 4: return fail("maxblock", True)
    if bd & 15: return fail("reserved", True)
    if (xxh32(read(4, hsize - 5)) >> 8) & 0xFF != read(hsize - 1, 1)[0]: return fail("headerck", True)
    r["flags"] = flg
    bs, bck = bs_of((bd >> 4) & 7), (flg >> 4) & 1
    declared = struct.unpack("<Q", read(6, 8))[0] if flg & 8 else 0
    table_cap = min(room // bs + 2, cap // 5 + 2)      # (the call's bound on the blocks: one per block size of room, one per 5 frame bytes)
    pos, blocks = hsize, []
    while True:
        if cap - pos < 4: return fail("incomplete")
        w = u32(read(pos, 4)); pos += 4
        if w == 0: break
        n = w & 0x7FFFFFFF
        if n > bs: return fail("maxblock")
        if cap - pos < n + 4 * bck: return fail("incomplete")
        if len(blocks) >= table_cap or len(blocks) * bs >= room: return fail("dstsmall")      # (block i decodes at i * block size)
        assert w & STORED, "the model knows stored blocks only"
        blocks.append((pos, n)); pos += n + 4 * bck
    if flg & 4:
        if cap - pos < 4: return fail("incomplete")
        pos += 4
    r.update(n_blocks=len(blocks), consumed=pos, size=declared)
    if bck and checks:
        for i, (p, n) in enumerate(blocks):
            if xxh32(read(p, n)) != u32(read(p + n, 4)):
                r.update(status=ST["blockck"], first_bad_block=i); return r
    total = sum(n for _, n in blocks)
    assert total <= room
    if flg & 8 and declared != total:
        r.update(status=ST["framesize"], size=total); return r
    r["size"] = total
    if flg & 4 and checks and xxh32(b"".join(read(p, n) for p, n in blocks)) != u32(read(pos - 4, 4)):
        r["status"] = ST["contentck"]
    return r


# ---- the cases ----------------------------------------------------------------------------------------------------------------
CASES = {}                             # name -> (builder, kwargs)


def reg(name, fn, **kw):
    assert name not in CASES, name
    CASES[name] = (fn, kw)


def case(name) -> Case:
    fn, kw = CASES[name]
    return fn(name, **kw)


def full(c, n): return [c.bs] * n
def n_par(bsid): return 17 if bsid == 4 else 5         # blocks that make a frame of just over 1 MiB


# -- parallel walk: sound frames
def par_plain(name, bsid, bck, cck, csize):
    c = Case(name, "parallel", bsid, bck, cck, csize)
    end = c.frame(full(c, n_par(bsid)))
    return c.done(end, "must_deliver", "parallel", ["par/full"])


def par_mixed(name, bsid):
    c = Case(name, "parallel", bsid, bck=1, cck=1)
    lens = full(c, n_par(bsid)) + [0, 1, c.bs - 1, c.bs, 0, 0, 1, int(c.rng.integers(2, c.bs - 1)), c.bs - 1, 1, 0, c.bs]
    order = c.rng.permutation(len(lens))
    end = c.frame([lens[i] for i in order])
    return c.done(end, "must_deliver", "parallel", ["par/mixed"])


def lens_word_at(c, n, k, target):
    """n full blocks, but the one in front of block k shortened so that block k's size word starts at `target`."""
    lens = full(c, n)
    natural = c.hsize + k * (c.bs + 4 + 4 * c.bck)
    assert 0 < natural - target <= c.bs
    lens[k - 1] -= natural - target
    return lens


def par_shift(name, seam, j, bck=0):
    c = Case(name, "parallel", 4, bck=bck)
    k, n = 6, 18
    natural = c.hsize + k * (c.bs + 4 + 4 * bck)
    edge = {"chunk": k * WK_CHUNK, "group": (natural // WK_GROUP - 5) * WK_GROUP, "stride": k * WK_CHUNK - 3 * WK_STRIDE}[seam]
    assert edge % {"chunk": WK_CHUNK, "group": WK_GROUP, "stride": WK_STRIDE}[seam] == 0 and (seam == "chunk" or edge % WK_CHUNK)
    assert seam != "group" or edge % WK_STRIDE
    end = c.frame(lens_word_at(c, n, k, edge + j))
    assert c.words[k] == edge + j
    return c.done(end, "must_deliver", "parallel", ["par/shift/%s" % seam])


def par_tail(name, last, cck=0):
    """The frame_cap ends right behind the frame: the last size word's bytes, or the EndMark's, lie in k_walk_cand's byte-wise tail."""
    c = Case(name, "parallel", 4, cck=cck)
    end = c.frame(full(c, 17) + [last])
    seams = ["par/cap/cck" if cck else "par/cap/endmark"]
    if end - (c.words[-1] + 3) <= WK_TAIL and not cck: seams.append("par/tail20")
    return c.done(end, "must_deliver", "parallel", seams)


def par_threshold(name, cap):
    c = Case(name, "parallel", 4)
    end = c.frame(full(c, 15) + [30000, 29000])
    assert end < PAR_MIN_CAP - 1
    return c.done(cap, "must_deliver" if cap >= PAR_MIN_CAP else "must_decline", "parallel" if cap >= PAR_MIN_CAP else "serial", ["par/threshold/%d" % cap])


def par_slots(name, n_in_chunk):
    """n_in_chunk true size words in the chunk that begins at 3 * WK_CHUNK."""
    c = Case(name, "parallel", 4)
    each = 2180
    first = lens_word_at(c, 4, 3, 3 * WK_CHUNK + 8)[:3]
    lens = first + [each] * (n_in_chunk - 1) + [c.bs] + full(c, 14)
    end = c.frame(lens)
    inside = [w for w in c.words if w // WK_CHUNK == 3]
    assert len(inside) == n_in_chunk and max(sum(1 for w in c.words if w // WK_CHUNK == q) for q in range(end // WK_CHUNK + 1) if q != 3) <= 2
    return c.done(end, "must_deliver" if n_in_chunk <= WK_SLOTS else "free", "parallel", ["par/slots/%d" % n_in_chunk])


def par_behind(name, what):
    c = Case(name, "parallel", 4, cck=1)
    end = c.frame(full(c, 17))
    expect, room = "must_deliver", None
    if what == "random":
        c.rand(end, 4096); cap = end + 4096
    elif what == "zeros":
        c.fill(end, 40000, 0); cap = end + 40000
    elif what == "chain":
        cap = c.chain(end, [5000, c.bs, 1, 70], first=False) + 100
    else:                               # more candidates than the list holds, and never more than WK_SLOTS in a chunk
        n2 = len(c.segs) + 2 + LIST_SLACK + 60
        cap = c.chain(end, [2200] * n2, first=False) + 16
        expect = "free"
    return c.done(cap, expect, "parallel", ["par/behind/%s" % what])


def decoy_word(c, target, lo=512, hi=32000, stored=None):
    """(position, word): a word `lo..hi` bytes in front of `target` whose block would end exactly there.  Its low byte is 1..0x7F and
    its second byte 2..0x7F, so that no word that overlaps it looks like a size word."""
    while True:
        v = int(c.rng.integers(lo, hi))
        if 1 <= (v & 0xFF) <= 0x7F and 2 <= (v >> 8) <= 0x7F: break
    st = int(c.rng.integers(0, 2)) if stored is None else stored
    return target - 4 - 4 * c.bck - v, v | (STORED if st else 0)


def par_decoy(name, what, bck=0):
    c = Case(name, "parallel", 4, bck=bck)
    end = c.frame(full(c, 18))
    W = c.words
    expect = "free"
    if what == "single":                # -> W[9] -> W[10] -> W[11]: WK_HOPS good hops; nobody points at it
        p, w = decoy_word(c, W[9]); c.put(p, le32(w)); c.decoys = [p]; expect = "must_deliver"
    elif what == "pair":                # A -> B -> W[9]
        pb, wb = decoy_word(c, W[9]); pa, wa = decoy_word(c, pb, hi=20000)
        c.put(pb, le32(wb)); c.put(pa, le32(wa)); c.decoys = [pa, pb]
    elif what == "pair_end":            # A -> B -> the true EndMark
        pb, wb = decoy_word(c, end - 4); pa, wa = decoy_word(c, pb, hi=20000)
        c.put(pb, le32(wb)); c.put(pa, le32(wa)); c.decoys = [pa, pb]
    else:                               # -> an EndMark planted in the payload
        z = W[9] - 20000
        p, w = decoy_word(c, z); c.put(z, le32(0)); c.put(p, le32(w)); c.decoys = [p]
    assert all(any(s <= d and d + 4 <= s + n for s, n in c.segs) for d in c.decoys), name
    return c.done(end, expect, "parallel", ["par/decoy/%s" % what])


def par_bad(name, what):
    c = Case(name, "parallel", 4, bck=1, cck=1)
    n, room, planned, at0 = 18, None, "parallel", 0
    kw = {}
    if what == "word_bs+1_stored": kw = dict(words={9: STORED | (c.bs + 1)})
    if what == "word_bs+1": kw = dict(words={9: c.bs + 1})
    if what == "skippable":
        c.put(0, le32(SKIP0 + 5) + le32(11) + b"eleven byte"); at0 = 19
    at = c.header(at=at0, content=0, wrong_hc=what == "header_checksum")
    end = c.chain(at, full(c, n), **kw)
    cap = end
    stride = c.bs + 8
    if what == "cut_payload": cap = at + 17 * stride + 4 + 12345
    if what == "cut_word": cap = at + 17 * stride + 2
    if what == "no_endmark": cap = end - 8
    if what == "no_cck": cap = end - 4
    if what == "room": room = (n - 1) * c.bs
    expect = "must_decline"
    if what == "block_checksum":        # (the walk is sound: the list may deliver; the record must name the block)
        c.ops.append(("late", c.words[9] + 4 + c.bs, b"\x01\x02\x03\x04")); expect = "free"
    c.ops = [op for op in c.ops if op[1] + (4 if op[0] == "xxh" else len(op[2])) <= cap]      # (what lies behind a cut is not there)
    if what == "skippable": c.segs, c.words, c.lens = [], [], []
    return c.done(cap, expect, planned, ["par/bad/%s" % what], room=room if room is not None else n * c.bs)


# -- seeded walk
def seed_geometry(c, cap):
    """(start of seed window s for s in 0..63, the window's length) as k_walk_seeds lays them out."""
    span = cap - c.hsize
    return [c.hsize + (span // WK_SEEDS) * s for s in range(WK_SEEDS)], c.bs + 64


def seeded(name, what, bsid=6, big=True):
    c = Case(name, "seeded", bsid)
    T = SEED_BLOCKS if big else SMALL_SEED_BLOCKS            # block sizes of frame_cap from which the seeded walk is planned
    bs, expect, planned, room = c.bs, "must_deliver", "parallel", None
    if what == "full":
        cap = c.frame(full(c, T + 1))
    elif what == "half":
        lens = []
        while sum(lens) < T * bs: lens.append(int(c.rng.integers(bs // 2, bs + 1)))
        cap = c.frame(lens)
    elif what in ("threshold-1", "threshold"):
        end = c.frame(full(c, T - 1))
        cap = T * bs - (1 if what == "threshold-1" else 0)
        assert end < cap
        if what == "threshold-1": expect, planned = "must_decline", "serial"
    elif what in ("short_zeros", "short_chain"):
        # a frame that ends in front of the first seed window; zeros behind it (no word of zeros is a candidate: it is an EndMark)
        n1 = 100 if big else 3
        end = c.frame([16384 if big else 9000] * n1)
        cap = T * bs + 4096
        win, _ = seed_geometry(c, cap)
        assert n1 < WK_LANE_CAP and end + 8 < win[1]
        if what == "short_zeros":
            c.fill(end, cap - end, 0)
        else:                           # a second chain that the seed windows do find; it must not join the first
            at2 = win[2] + 1000
            c.fill(end, at2 - end, 0)
            end2 = c.chain(at2, full(c, 5 if big else 1) + [777], first=False)
            assert end2 < cap
            c.fill(end2, cap - end2, 0)
    elif what == "lane_cap":
        # more than WK_LANE_CAP small blocks behind the last seed window: the last lane's stretch overflows
        nfull = T - 2
        lens = full(c, nfull) + [4096] * (WK_LANE_CAP + 8)
        end = c.frame(lens)
        cap = max(end, T * bs + 64)
        win, _ = seed_geometry(c, cap)
        if big: assert c.words[nfull] > win[-1] and c.words[nfull - 1] >= win[-1], (c.words[nfull], win[-1])
        expect = "free"
    elif what == "window_decoy":
        cap = c.frame(full(c, T + 1))
        win, _ = seed_geometry(c, cap)
        a = win[20]
        m = min(w for w in c.words if w > a + 600)
        assert not any(w - 4 < a < w + 4 for w in c.words) and m - a - 4 <= bs
        c.put(a, le32((m - a - 4) | STORED)); c.decoys = [a]
        expect = "free"
    elif what == "seed_list":
        cap = c.frame(full(c, T + 1))
        win, _ = seed_geometry(c, cap)
        a = (win[10] + 64) & ~3
        nw = WK_SEED_LIST + 1000
        assert not any(a - 8 < w < a + 4 * nw + 8 for w in c.words) and 4 * nw < WK_SEED_PIECE
        lo = c.rng.integers(1, 0x80, nw, dtype=np.uint8); hi = c.rng.integers(1, 0x80, nw, dtype=np.uint8)
        c.put(a, b"".join(bytes([int(x), int(y), 0, 0]) for x, y in zip(lo, hi)))
        expect = "free"
    elif what == "cut_payload":
        end = c.frame(full(c, T + 6))
        cap = c.words[T + 4] + 4 + bs // 3
        assert cap >= T * bs
        c.ops = [op for op in c.ops if op[1] + len(op[2]) <= cap]
        expect, room = "must_decline", (T + 6) * bs
    elif what == "word_bs+1":
        cap = c.frame(full(c, T + 1), words={T // 2: STORED | (bs + 1)})
        expect, room = "must_decline", (T + 1) * bs
    elif what == "no_endmark":
        cap = c.frame(full(c, T + 1), endmark=False)
        expect, room = "must_decline", (T + 1) * bs
    else:
        raise KeyError(what)
    if planned == "parallel": assert bs > PAR_MAX_BS and cap >= T * bs, (name, cap)
    c.big = big
    c.cap, c.expect, c.planned, c.seams = cap, expect, planned, ["seed/%s%s" % (what, "/bsid7" if bsid == 7 else "")]
    c.room = len(c.segs) * bs if room is None else room
    return c


def seeded_small(name) -> Case:
    """The recipe of a seeded case at a few blocks, for the CPU test."""
    fn, kw = CASES[name]
    assert fn is seeded
    return seeded(name, **dict(kw, big=False))


# -- trailer walk
def trailer_bytes(F: int, entries, count=None) -> bytes:
    """lz4f_mi355x.h, "the trailer": a skippable frame behind a frame of F bytes - magic, size, pad to 16, one u64 per block (an even
    number of them), a 32-byte footer that ends the stream."""
    n = len(entries) if count is None else count
    list_at = (F + 8 + 15) & ~15
    n_list = (n + 1) & ~1
    total = list_at + n_list * 8 + 32 - F
    e = list(entries)[:n_list] + [0] * (n_list - len(entries))
    return (le32(TR_MAGIC) + le32(total - 8) + bytes(list_at - F - 8) + b"".join(le64(x) for x in e) +
            struct.pack("<IIIIIIQ", 0, 0, 0, 0, TR_FOOT, n, total))


def trailer_lens(c, salt=0):
    r = np.random.Generator(np.random.PCG64(zlib.crc32(("trailer lens %d %d" % (c.bsid, salt)).encode())))
    return [int(x) for x in r.integers(1000, 60000, 5)]


def trailer(name, bsid, lie):
    c = Case(name, "trailer", bsid, bck=1, cck=1)
    F = c.frame(trailer_lens(c))
    W, n = list(c.words), len(c.words)
    expect = "must_decline"
    if lie == "bare":
        return c.done(F, "must_decline", "serial", ["trailer/bare"])
    if lie == "honest": e, expect = W, "must_deliver"
    elif lie == "+1": e = W[:2] + [W[2] + 1] + W[3:]
    elif lie == "-1": e = W[:2] + [W[2] - 1] + W[3:]
    elif lie == "swapped": e = W[:1] + [W[2], W[1]] + W[3:]
    elif lie == "duplicated": e = W[:2] + [W[1]] + W[3:]
    elif lie == "2^64-1": e = W[:3] + [(1 << 64) - 1] + W[4:]
    elif lie == "cap-3": e = None
    elif lie == "count+1": e = W + [F - (8 if c.cck else 4)]          # (the extra entry: the EndMark)
    elif lie == "count-1": e = W[:-1]
    elif lie == "first": e = [W[0] + 4] + W[1:]
    elif lie == "other_frame":
        o = Case(name + " (other)", "trailer", bsid, bck=1, cck=1)
        o.frame(trailer_lens(c, salt=1))
        e = list(o.words)
        assert len(e) == n and e != W
    else: raise KeyError(lie)
    if lie == "cap-3":
        cap = F + len(trailer_bytes(F, W))
        e = W[:3] + [cap - 3] + W[4:]
    t = trailer_bytes(F, e)
    c.put(F, t)
    c.bare = "trailer/bsid%d/bare" % bsid
    return c.done(F + len(t), expect, "trailer", ["trailer/%s" % lie])


for _bsid in (4, 5):
    for _b in (0, 1):
        for _k in (0, 1):
            for _s in (0, 1):
                reg("par/full/bsid%d/b%dk%ds%d" % (_bsid, _b, _k, _s), par_plain, bsid=_bsid, bck=_b, cck=_k, csize=_s)
    reg("par/mixed/bsid%d" % _bsid, par_mixed, bsid=_bsid)
for _seam in ("chunk", "group", "stride"):
    for _j in (-3, -2, -1, 0):
        reg("par/shift/%s%+d" % (_seam, _j), par_shift, seam=_seam, j=_j, bck=1 if _j == -2 else 0)
for _last in (1, 8, 12):
    reg("par/tail20/last%d" % _last, par_tail, last=_last)
reg("par/cap/endmark", par_tail, last=4000)
reg("par/cap/cck", par_tail, last=4000, cck=1)
reg("par/threshold/2^20-1", par_threshold, cap=PAR_MIN_CAP - 1)
reg("par/threshold/2^20", par_threshold, cap=PAR_MIN_CAP)
reg("par/slots/30", par_slots, n_in_chunk=WK_SLOTS)
reg("par/slots/31", par_slots, n_in_chunk=WK_SLOTS + 1)
for _w in ("random", "zeros", "chain", "long_chain"):
    reg("par/behind/%s" % _w, par_behind, what=_w)
for _w in ("single", "pair", "pair_end", "endmark"):
    reg("par/decoy/%s" % _w, par_decoy, what=_w)
reg("par/decoy/single/bck", par_decoy, what="single", bck=1)
PAR_BAD = ("cut_payload", "cut_word", "no_endmark", "no_cck", "word_bs+1_stored", "word_bs+1", "header_checksum", "skippable", "room", "block_checksum")
for _w in PAR_BAD:
    reg("par/bad/%s" % _w, par_bad, what=_w)
SEEDED = ("full", "half", "threshold-1", "threshold", "short_zeros", "short_chain", "lane_cap", "window_decoy", "seed_list", "cut_payload", "word_bs+1",
          "no_endmark")
for _w in SEEDED:
    reg("seed/%s" % _w, seeded, what=_w)
reg("seed/full/bsid7", seeded, what="full", bsid=7)
LIES = ("+1", "-1", "swapped", "duplicated", "2^64-1", "cap-3", "count+1", "count-1", "first", "other_frame")
for _bsid in (4, 7):
    for _l in ("bare", "honest") + LIES:
        reg("trailer/bsid%d/%s" % (_bsid, _l), trailer, bsid=_bsid, lie=_l)

# The expectations, by name.  must_deliver: the guessed list is the chain, so LZ4F_MI355X_PATH_WALK_DELIVERED must be set.
# must_decline: the frame is malformed, the list lies, or no guessing walk is planned - the bit must be clear.  free: the design
# allows either (an overflow exit, a decoy that is pointed at, a sound walk in front of a bad block): only equality is asserted.
FREE = {"par/slots/31", "par/behind/long_chain", "par/decoy/pair", "par/decoy/pair_end", "par/decoy/endmark", "par/bad/block_checksum",
        "seed/lane_cap", "seed/window_decoy", "seed/seed_list"}
MUST_DECLINE = ({"par/threshold/2^20-1", "seed/threshold-1", "seed/cut_payload", "seed/word_bs+1", "seed/no_endmark"} |
                {"par/bad/%s" % w for w in PAR_BAD if w != "block_checksum"} |
                {"trailer/bsid%d/%s" % (b, l) for b in (4, 7) for l in ("bare",) + LIES})
MUST_DELIVER = set(CASES) - FREE - MUST_DECLINE

# every seam the cases are there for: the CPU test holds the list to this inventory
SEAMS = (["par/full", "par/mixed", "par/shift/chunk", "par/shift/group", "par/shift/stride", "par/tail20", "par/cap/endmark", "par/cap/cck",
          "par/threshold/%d" % (PAR_MIN_CAP - 1), "par/threshold/%d" % PAR_MIN_CAP, "par/slots/%d" % WK_SLOTS, "par/slots/%d" % (WK_SLOTS + 1)] +
         ["par/behind/%s" % w for w in ("random", "zeros", "chain", "long_chain")] + ["par/decoy/%s" % w for w in ("single", "pair", "pair_end", "endmark")] +
         ["par/bad/%s" % w for w in PAR_BAD] + ["seed/%s" % w for w in SEEDED] + ["seed/full/bsid7", "trailer/bare", "trailer/honest"] +
         ["trailer/%s" % l for l in LIES])


def names(kind=None):
    return [n for n in CASES if kind is None or n.split("/")[0] == kind]
