"""Planted guesses for the stretch self-index (csrc/decode_spx.cuh, k_spx_index): a corpus of named, valid LZ4 frames of big
independent blocks whose payloads put a byte pattern on every decision the kernel's four steps make (test helper, not a test
module).  tests/spx_model.py says what the kernel must make of each; every case carries `want`, predicates over that verdict, so
a builder that drifts off its seam fails tests/test_spx_model_cpu.py rather than silently testing something else.

How payloads are laid out.  Literal bytes are below 0xF0 and offsets below 0xF000, so the only "0xF? 0xFF" pairs of a payload
are planted ones: a true token with 270 literals or more, or bytes written into a literal run on purpose.  The background is
sequences of 120 literals and a 4-byte match (124 payload bytes, 124 output bytes), with a token laid exactly on every multiple
of SPX_SEG, so a lane that finds no pair starts blind ON a true token and every lane lands on the next one's start: whatever a
case plants is the only thing that disturbs the stitch.  Seeds are the CRC32 of the case's name.

Families (the name's first word):
  lanes     csize on both sides of spx_lanes' thresholds 1->2, 2->3, 127->128 lanes, and a payload of exactly 4 MiB
  pairs     a true long-literal token at segment offsets 0, 15, 16 (the byte behind a scan lane's sixteen), 1023, 1024 (two
            loads), SPX_SCAN - 1 (its second byte is outside the scanned bytes) and SPX_SCAN (unseen: the lane starts blind); one in
            lane 70's segment (the workgroup's second wave scans it), found by scan lane 37; the last lane of the smallest payload that has it, with its pair in the scan's last KiB.  (The scan's own bound,
            a + 1024 + 24 < csize, cannot cut a scan short: a lane exists only with SPX_SCAN + 2048 bytes behind its segment's start;
            test_spx_model_cpu.py states that arithmetic.)
  cand      0..7 decoy pairs (literal bytes, or the offset 0xFFF0) in front of the true token in one KiB: the true token in place
            SPX_CAND is taken, in place SPX_CAND + 1 the lane stays out; decoys in one KiB and the token in a later one: out
  decoy     a fake token inside a literal run that passes spx_likely_token; its chain falls into step, runs into a non-sequence,
            "ends" at csize (at once, or a hop later), crawls into the by_pair exit, or passes over the next lane's start.  The
            lane in front overshoots the fake start and the stitching thread walks
  over      literal runs of one, two and three and a half segments, inside the block and as its last sequence
  notes     lane 0 and lane 1 with exactly 15..257 sequences to the next start; a note taken on the block's last token
  exits     by_pair with 31 / 32 long tokens among a pair-started true lane's first 63; slow (density words given) on both sides
            of bytes_per_seq / 8; the hop cap with SPX_LANE_HOPS, one and two more sequences to the next start
  rescue    the stitching thread walks exactly SPX_RESCUE sequences, and one more, in one block; lanes kept out by decoy pairs
  mixed     256 KiB blocks: stored blocks between compressed ones, a short last block, block checksums
`declines_probe` / `declines` say which cases the kernel is expected to decline with / without the case's density words.
"""
from __future__ import annotations

import zlib

import numpy as np

import lz4_grammar as G
import spx_model as S

SEG, SCAN, CAND = S.SEG, S.SCAN, S.CAND
PER = 124


def hdr(lit): return 1 + (0 if lit < 15 else 1 + (lit - 15) // 255)


def lit_for(size):
    """Literals of a sequence (no match-length byte) that takes `size` payload bytes, or None."""
    for h in range(1, 64):
        lit = size - 2 - h
        if lit >= 0 and hdr(lit) == h: return lit
    return None


class Case:
    def __init__(self, name, bsid=7, bck=False, density=None, aim=""):
        self.name, self.aim, self.density = name, aim, density
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.fr = G.Frame(bsid, bck=bck)
        self.b, self.want, self.at = None, [], {}
        self._after = []                                  # (payload position, bytes, mark): written into the first literal run that starts there or later
        self.declines = self.declines_probe = False

    @property
    def family(self): return self.name.split("/")[0]
    @property
    def pos(self): return len(self.b.body)
    @property
    def op(self): return self.b.op

    def blk(self):
        self.b = self.fr.block()
        return self

    def need(self, what, fn): self.want.append((what, fn))

    def lit(self, n): return self.rng.integers(0, 0xF0, n, dtype=np.uint8).tobytes()

    def plant_after(self, at, data, mark):
        self._after.append((at, data, mark)); self._after.sort()

    def s(self, lit, ml=4, off=None, mark=None):
        """One sequence; lit: a count or the bytes.  Returns the payload position of its token."""
        data = bytearray(self.lit(lit) if isinstance(lit, int) else lit)
        n, at = len(data), self.pos
        p0 = at + hdr(n)
        if self._after and p0 >= self._after[0][0] and n >= len(self._after[0][1]) + 2:
            _, d, m = self._after.pop(0)
            data[0:len(d)] = d
            self.at[m] = p0
        if off is None: off = min(self.op + n, 0x0820)
        assert ml >= 4 and 0 < off <= self.op + n, (self.name, at, n, ml, off)
        self.b.s(bytes(data), ml, off)
        if mark: self.at[mark] = at
        return at

    def q(self, size, mark=None):
        lit = lit_for(size)
        assert lit is not None and (lit or self.op), (self.name, size)
        return self.s(lit, mark=mark)

    def long(self, lit=300, mark=None):
        assert lit >= 270
        return self.s(lit, mark=mark)

    def fill_to(self, target, per=PER):
        while True:
            r = target - self.pos
            if r == 0: return
            assert r >= 3, (self.name, target, r)
            if r > 273: self.q(min(per, r - 30))
            elif lit_for(r) is not None and (lit_for(r) or self.op): self.q(r)
            else: self.q(r // 2)                          # (18 bytes: no single sequence is that long)

    def plain_to(self, target, per=PER):
        """Background up to payload position `target`, a token on every multiple of SPX_SEG on the way."""
        while self.pos < target:
            nxt = (self.pos // SEG + 1) * SEG
            self.fill_to(min(nxt, target), per)

    def exact(self, nseq, target):
        """Exactly nseq sequences that end at payload position `target`."""
        total = target - self.pos
        per, r = divmod(total, nseq)
        sizes = [per + 1] * r + [per] * (nseq - r)
        for _ in range(8):
            bad = [i for i, v in enumerate(sizes) if lit_for(v) is None]
            if not bad: break
            for i in bad:
                j = next(j for j in range(len(sizes)) if j != i and lit_for(sizes[j]) is not None and lit_for(sizes[j] - 1) is not None and sizes[j] - 1 >= 4)
                sizes[i] += 1; sizes[j] -= 1
        assert sum(sizes) == total and all(lit_for(v) is not None for v in sizes), (self.name, nseq, total)
        order = self.rng.permutation(len(sizes))
        for i in order: self.q(sizes[int(i)])
        assert self.pos == target

    def end_at(self, csize):
        """The block's last sequence, so that the payload has exactly csize bytes."""
        r = csize - self.pos
        assert 20 <= r <= 260, (self.name, r)
        self.end(r - 2)

    def end(self, n):
        assert not self._after, (self.name, "a plant found no literal run", self._after)
        self.b.end(self.lit(n) if isinstance(n, int) else n); self.b = None

    def finish(self, csize):
        self.plain_to(csize - 100); self.end_at(csize)

    def full(self):
        """Close a block that decodes to exactly the frame's block size."""
        bs = self.fr.bs
        self.s(120, ml=60)                                # (56 output bytes more than payload bytes: the payload stays under the block size)
        while bs - self.op > 700:
            nxt = (self.pos // SEG + 1) * SEG
            if nxt - self.pos > 2 * PER + 30: self.q(PER)
            else: self.fill_to(nxt)
        self.end(bs - self.op)


def payloads(fb: bytes):
    """[(src_off, word)] of a frame's blocks (no content size, no dictionary id in these frames)."""
    import struct
    out, pos, bck = [], 7, (fb[4] >> 4) & 1
    while True:
        w = struct.unpack_from("<I", fb, pos)[0]; pos += 4
        if w == 0: return out
        out.append((pos, w)); pos += (w & 0x7FFFFFFF) + 4 * bck


def lane(m, u): return m[0]["lanes"][u]          # (m: the model's verdict per compressed block; most cases have one block)


# ------------------------------------------------------------------------------------------------------------------------
def _lanes():
    T = SEG + SCAN + 2048
    for tag, csize, n in (("1", T, 1), ("2", T + 1, 2), ("2top", 2 * SEG + SCAN + 2048, 2), ("3", 2 * SEG + SCAN + 2049, 3),
                          ("127", 126 * SEG + SEG + SCAN + 2048, 127), ("128", 127 * SEG + SCAN + 2049, 128), ("4mib", 4 << 20, 128)):
        c = Case("lanes/" + tag, aim="spx_lanes: %d bytes of payload are %d lanes" % (csize, n))
        c.blk(); c.finish(csize)
        c.need("csize and lanes", lambda m, c, csize=csize, n=n: len(m[0]["lanes"]) == n and S.lanes(csize) == n and m[0]["points"][-1][0] == csize)
        c.need("every lane is true and nothing is walked by the stitch", lambda m, c: all(l["true"] for l in m[0]["lanes"]) and m[0]["stitched"] == 0)
        yield c


def _pairs():
    for off in (0, 15, 16, 1023, 1024, SCAN - 1, SCAN):
        c = Case("pairs/off%d" % off, aim="the pair scan: a true long-literal token %d bytes into lane 1's segment" % off)
        c.blk(); c.plain_to(SEG); c.fill_to(SEG + off)
        c.long(mark="t1"); c.long(mark="t2")
        c.finish(2 * SEG + SCAN + 2049 + 3000)
        seen = off < SCAN
        c.need("the token is where it was aimed", lambda m, c, off=off: c.at["t1"] == SEG + off)
        c.need("lane 1 starts at the token iff the scan sees it; blind at its segment's start otherwise",
               lambda m, c, off=off, seen=seen: lane(m, 1)["start"] == (SEG + off if seen else SEG) and (SEG + off in lane(m, 1)["cand"]) == seen)
        c.need("lane 1 is true, lane 0 lands on it", lambda m, c: lane(m, 1)["true"] and lane(m, 0)["landing"][0] == lane(m, 1)["start"] and m[0]["stitched"] == 0)
        yield c
    u, off = 70, 16 * 37 + 5
    c = Case("pairs/second_wave", aim="the pair scan of the workgroup's second wave: a true long-literal token in lane %d's segment, byte 5 of scan lane 37" % u)
    c.blk(); c.plain_to(u * SEG); c.fill_to(u * SEG + off)
    c.long(mark="t1"); c.long(mark="t2")
    c.finish((u + 1) * SEG + SCAN + 2049 + 3000)
    c.need("lane %d starts at the token and is true, nothing is walked by the stitch" % u, lambda m, c, u=u, off=off: c.at["t1"] == u * SEG + off and lane(m, u)["start"] == c.at["t1"] and
           lane(m, u)["cand"] == [c.at["t1"], c.at["t2"]] and all(l["true"] for l in m[0]["lanes"]) and m[0]["stitched"] == 0)
    yield c
    csize = SEG + SCAN + 2049
    c = Case("pairs/last_lane_last_kib", aim="the last lane of the smallest payload that has two, its pair in the scan's last KiB")
    c.blk(); c.plain_to(SEG); c.fill_to(SEG + SCAN - 500)
    c.long(mark="t1"); c.long(mark="t2")
    c.finish(csize)
    c.need("lane 1 reads 8 KiB and starts at the token", lambda m, c: len(m[0]["lanes"]) == 2 and lane(m, 1)["kib"] == 8 and lane(m, 1)["start"] == c.at["t1"] and lane(m, 1)["true"])
    yield c


def _cand():
    for k in range(8):
        c = Case("cand/decoys%d" % k, aim="the candidate list: %d pairs that are no tokens in front of the true one, in one KiB" % k)
        c.blk(); c.plain_to(3 * SEG)
        ds = []
        for i in range(k):
            at0 = c.pos
            if i % 2 == 0:
                d = bytearray(c.lit(60)); d[20:23] = b"\xF5\xFF\x33"
                c.s(bytes(d)); ds.append(at0 + 2 + 20)
            else:
                c.s(60, off=0xFFF0); ds.append(at0 + 2 + 60)
        c.fill_to(3 * SEG + 600)
        c.long(mark="t1"); c.long(350, mark="t2")
        c.finish(4 * SEG + SCAN + 2049 + 5000)
        taken = k < CAND
        c.need("the decoys lead the list in position order, cut at SPX_CAND", lambda m, c, ds=ds, k=k: lane(m, 3)["cand"] == (ds + [c.at["t1"], c.at["t2"]])[:CAND] and lane(m, 3)["kib"] == 1)
        c.need("the true token in place %d: %s" % (k + 1, "taken" if taken else "the lane stays out"),
               lambda m, c, taken=taken: lane(m, 3)["start"] == (c.at["t1"] if taken else None) and lane(m, 3)["true"] == taken and lane(m, 4)["true"])
        if not taken: c.need("lane 2 walks through lane 3's stretch to lane 4", lambda m, c: lane(m, 2)["landing"][0] == 4 * SEG and m[0]["stitched"] == 0)
        yield c
    c = Case("cand/later_kib", aim="a decoy in one KiB, the true token two KiB later: the scan stops at the first KiB that shows a pair")
    c.blk(); c.plain_to(3 * SEG)
    d = bytearray(c.lit(60)); d[20:23] = b"\xF5\xFF\x33"
    c.s(bytes(d)); c.fill_to(3 * SEG + 2500)
    c.long(mark="t1"); c.long(mark="t2")
    c.finish(4 * SEG + SCAN + 2049 + 5000)
    c.need("one candidate, one KiB, the lane stays out", lambda m, c: lane(m, 3)["cand"] == [3 * SEG + 22] and lane(m, 3)["kib"] == 1 and lane(m, 3)["start"] is None and not lane(m, 3)["true"])
    yield c


def _fake(c, start, run, d_at, pieces):
    """A true sequence at `start` with `run` literals; `pieces`: {position in the payload: bytes} written into them."""
    data = bytearray(c.lit(run))
    p0 = start + hdr(run)
    for at, bts in pieces.items():
        assert p0 <= at and at + len(bts) <= p0 + run, (c.name, at, p0, run)
        data[at - p0:at - p0 + len(bts)] = bts
    assert c.pos == start
    c.s(bytes(data), mark="s0")
    return p0 + run                                       # where the literals end (the true offset's first byte)


def _decoy():
    aim = "a wrong guess that spx_likely_token lets through: "
    # -- the fake chain falls into step: its first sequence ends where the true one's literals end, so its second token is the true next token
    c = Case("decoy/in_step", aim=aim + "the fake sequence shares the true one's offset bytes and the chain is true from the next token on")
    c.blk(); c.plain_to(SEG); c.fill_to(2 * SEG - 100)
    run = 600
    lend = 2 * SEG - 100 + hdr(run) + run
    d = 2 * SEG + 40
    _fake(c, 2 * SEG - 100, run, d, {d: bytes([0xF0, 0xFF, lend - d - 273])})
    c.long(mark="t1")
    c.finish(3 * SEG + SCAN + 2049 + 3000)
    c.need("lane 2 starts at the fake token and lands on lane 3's start", lambda m, c, d=d: lane(m, 2)["start"] == d and lane(m, 2)["fate"] == "landed" and lane(m, 2)["landing"][0] == 3 * SEG and not lane(m, 2)["true"])
    c.need("lane 1 passes over it and the stitching thread walks to lane 3", lambda m, c, d=d: lane(m, 1)["landing"][0] == c.at["t1"] > d and m[0]["stitched"] == 1 and lane(m, 3)["true"])
    yield c
    # -- the last lane's fake chain: runs into a non-sequence / ends at csize at once / ends at csize a hop later
    for kind in ("ran_into", "ends_at_once", "ends_later"):
        c = Case("decoy/" + kind, aim=aim + "the last lane's fake chain " + kind.replace("_", " "))
        csize = SEG + SCAN + 2049 + 2000
        c.blk(); c.plain_to(SEG - 100)
        run, d = 1400, SEG + 40
        pieces = {}
        if kind == "ends_at_once":
            k = next(k for k in range(1, 80) if 0 <= csize - (d + 2 + k) - 15 - 255 * k < 255)
            pieces[d] = bytes([0xF0]) + b"\xFF" * k + bytes([csize - (d + 2 + k) - 15 - 255 * k])
        else:
            p2 = d + 3 + 270 + 7 + 2                       # the fake sequence: 277 literals, an offset, then the next fake token
            pieces[d] = bytes([0xF0, 0xFF, 7])
            if kind == "ran_into": pieces[p2] = bytes([0xF0]) + b"\xFF" * 60 + bytes([1])      # 15 316 literals: more than the payload has left
            else:
                k = next(k for k in range(1, 80) if 0 <= csize - (p2 + 2 + k) - 15 - 255 * k < 255)
                pieces[p2] = bytes([0xF0]) + b"\xFF" * k + bytes([csize - (p2 + 2 + k) - 15 - 255 * k])
        _fake(c, SEG - 100, run, d, pieces)
        c.finish(csize)
        fate = "ran_into" if kind == "ran_into" else "ended"
        c.need("lane 1 (the last) starts at the fake token: " + fate, lambda m, c, d=d, fate=fate, kind=kind: len(m[0]["lanes"]) == 2 and lane(m, 1)["start"] == d and lane(m, 1)["fate"] == fate and
               lane(m, 1)["hops"] == {"ran_into": 1, "ends_at_once": 0, "ends_later": 1}[kind] and not lane(m, 1)["true"])
        c.need("lane 0 passes over it and the stitching thread walks to the end", lambda m, c, d=d: lane(m, 0)["landing"][0] > d and m[0]["stitched"] == 1 and not m[0]["gave_up"])
        yield c
    # -- crawls into the by_pair exit / passes over the next lane's start
    for kind in ("crawls", "passes_over"):
        c = Case("decoy/" + kind, aim=aim + "the fake chain " + ("crawls through a literal run until the by_pair rule stops it" if kind == "crawls" else "jumps over the next lane's start"))
        c.blk(); c.plain_to(SEG); c.fill_to(2 * SEG - 100)
        run, d = 4000, 2 * SEG + 40
        p2 = d + 3 + 270 + 7 + 2
        pieces = {d: bytes([0xF0, 0xFF, 7])}
        pieces[p2] = bytes([0xF0, 0xFF, 9]) if kind == "crawls" else bytes([0xF0]) + b"\xFF" * 130 + bytes([1])     # 33 166 literals
        _fake(c, 2 * SEG - 100, run, d, pieces)
        c.finish(3 * SEG + SCAN + 2049 + (3000 if kind == "crawls" else 6000))
        if kind == "crawls":
            c.need("lane 2 starts at the fake token and gives up at hop 63 by the by_pair rule", lambda m, c, d=d: lane(m, 2)["start"] == d and lane(m, 2)["fate"] == "by_pair" and lane(m, 2)["hops"] == 63 and not lane(m, 2)["true"])
        else:
            c.need("lane 2 starts at the fake token and lands behind lane 3's start", lambda m, c, d=d: lane(m, 2)["start"] == d and lane(m, 2)["fate"] == "landed" and lane(m, 2)["landing"][0] > 3 * SEG and lane(m, 2)["hops"] == 2)
        c.need("lane 1 passes over it and the stitching thread walks to lane 3", lambda m, c, d=d: lane(m, 1)["landing"][0] > d and m[0]["stitched"] == 1 and lane(m, 3)["true"] and not m[0]["gave_up"])
        yield c


def _over():
    for tag, run in (("1seg", SEG + 5000), ("2seg", 2 * SEG + 5000), ("3seg", 3 * SEG + SEG // 2)):
        for last in (False, True):
            c = Case("over/%s/%s" % (tag, "last" if last else "mid"), aim="a literal run of %d bytes %s: the lanes that start inside it lie behind the true chain" % (run, "as the block's last sequence" if last else "inside the block"))
            c.blk(); c.plain_to(SEG); c.fill_to(SEG + 9000)
            if last:
                c.at["t"] = c.pos
                c.end(run)
            else:
                c.long(run, mark="t")
                e = c.pos
                c.finish(((e + SEG - 1) // SEG + 1) * SEG + SCAN + 2049 + 1000)
            inside = lambda m, c, run=run: [u for u, l in enumerate(m[0]["lanes"]) if c.at["t"] < u * SEG < c.at["t"] + run]
            c.need("lanes start inside the run and none of them is true", lambda m, c, inside=inside, run=run: len(inside(m, c)) >= run // SEG and not any(lane(m, u)["true"] for u in inside(m, c)))
            if last: c.need("lane 1 ends the block", lambda m, c: lane(m, 1)["fate"] == "ended" and lane(m, 1)["true"] and m[0]["stitched"] == 0 and not m[0]["gave_up"])
            else: c.need("lane 1 lands behind the run, the stitching thread walks to the next lane, which is true",
                         lambda m, c, inside=inside, run=run: lane(m, 1)["landing"][0] > c.at["t"] + run and m[0]["stitched"] == 1 and lane(m, inside(m, c)[-1] + 1)["true"] and not m[0]["gave_up"])
            yield c


NOTE_COUNTS = {15: 0, 16: 0, 17: 1, 127: 7, 128: 7, 129: 8, 144: 8, 145: 4, 255: 7, 256: 7, 257: 8}


def _notes():
    for n, notes in NOTE_COUNTS.items():
        c = Case("notes/seqs%d" % n, aim="lane 0 and lane 1 with exactly %d sequences to the next lane's start: %d notes" % (n, notes))
        c.blk(); c.exact(n, SEG); c.exact(n, 2 * SEG)
        c.finish(2 * SEG + SCAN + 2049 + 2000)

        def chk(m, c, n=n, notes=notes):
            stride = 16 if n <= 144 else 32
            for u in (0, 1):
                l = lane(m, u)
                if not (l["true"] and l["hops"] == n and l["landing"] == (l["start"] + SEG, n, l["landing"][2]) and len(l["notes"]) == notes): return False
                if [s for _, s, _ in l["notes"]] != [stride * (i + 1) for i in range(notes)]: return False
            return m[0]["nr"] == 3 + 2 * notes + len(lane(m, 2)["notes"]) and m[0]["stitched"] == 0
        c.need("both lanes make n hops, keep the notes the stride leaves, and the points are the three starts and the notes", chk)
        yield c
    c = Case("notes/on_last_token", aim="one lane, sixteen sequences and the last: the note taken at hop 16 is the block's last token")
    c.blk(); c.exact(16, 4000); c.at["last"] = c.pos; c.end(50)
    c.need("the last token is a point", lambda m, c: m[0]["nr"] == 2 and m[0]["points"][1] == (c.at["last"], 16, m[0]["points"][1][2]) and lane(m, 0)["fate"] == "ended" and m[0]["cnt"] == 17)
    yield c


def _exits():
    # -- by_pair: a TRUE lane that started at a pair, 31 / 32 tokens with a literal nibble of 15 among its first 63
    for longs in (31, 32):
        c = Case("exits/by_pair/longs%d" % longs, aim="the by_pair rule at hop 63 with %d long tokens: %s" % (longs, "the true lane gives up and the frame is declined" if longs < 32 else "the lane goes on"))
        c.blk(); c.plain_to(SEG); c.fill_to(SEG + 100)
        c.long(mark="t1"); c.long(mark="t2")
        for _ in range(longs - 2): c.q(PER)
        for _ in range(63 - longs): c.q(10)
        c.finish(2 * SEG + SCAN + 2049 + 2000)
        c.declines = c.declines_probe = longs < 32
        if longs < 32: c.need("lane 1 is true and gives up: declined", lambda m, c: lane(m, 1)["start"] == c.at["t1"] and lane(m, 1)["fate"] == "by_pair" and lane(m, 1)["hops"] == 63 and lane(m, 1)["true"] and m[0]["gave_up"])
        else: c.need("lane 1 is true and lands on lane 2", lambda m, c: lane(m, 1)["start"] == c.at["t1"] and lane(m, 1)["fate"] == "landed" and lane(m, 1)["true"] and lane(m, 2)["true"] and not m[0]["gave_up"])
        yield c
    # -- slow: a blind true lane that makes 63 * (bytes_per_seq / 8) bytes in 63 hops, or one byte less
    for short in (0, 1):
        c = Case("exits/slow/%s" % ("under" if short else "at"), density=(1, 807), aim="the slow rule at hop 63 (bytes_per_seq 807: 100 bytes a hop): %d bytes made" % (6300 - short))
        c.blk(); c.plain_to(SEG)
        c.exact(63, SEG + 6300 - short)
        c.finish(2 * SEG + SCAN + 2049 + 2000)
        c.declines_probe = bool(short)
        c.need("lane 1 is blind and true; with the density words it %s" % ("gives up: declined" if short else "goes on"),
               lambda m, c, short=short: lane(m, 1)["start"] == SEG and lane(m, 1)["cand"] == [] and lane(m, 1)["true"] and lane(m, 1)["fate"] == ("slow" if short else "landed") and m[0]["gave_up"] == bool(short))
        yield c
    # -- the hop cap
    for u in (0, 1):
        for n in ((2048, 2049, 2050) if u == 0 else (2049, 2050)):
            c = Case("exits/hops/lane%d/seqs%d" % (u, n), aim="lane %d with %d sequences to the next lane's start (SPX_LANE_HOPS = 2048: 2049 steps are made)" % (u, n))
            c.blk()
            if u: c.plain_to(SEG)
            c.exact(n, (u + 1) * SEG)
            c.finish((u + 1) * SEG + SCAN + 2049 + 2000)
            c.declines = c.declines_probe = n > 2049
            c.need("the lane is true and %s" % ("lands" if n <= 2049 else "gives up: declined"),
                   lambda m, c, u=u, n=n: lane(m, u)["true"] and lane(m, u)["fate"] == ("landed" if n <= 2049 else "hops") and m[0]["gave_up"] == (n > 2049) and (n > 2049 or lane(m, u)["hops"] == n))
            yield c


def _rescue():
    for extra in (0, 1):
        n = S.RESCUE + extra
        c = Case("rescue/seqs%d" % n, aim="the stitching thread walks %d sequences in one block (SPX_RESCUE = %d)" % (n, S.RESCUE))
        K = 65
        c.blk(); c.plain_to(SEG - 60); c.q(PER, mark="x0")                # (a sequence across lane 1's blind start: lane 1 is a wrong guess)
        x = c.pos
        for u in range(2, K): c.plant_after(u * SEG + 64, b"\xF5\xFF\x33", "d%d" % u)
        c.exact(n, K * SEG)
        c.finish(K * SEG + SCAN + 2049 + 2000)
        c.declines = c.declines_probe = bool(extra)
        c.need("lanes 2..%d stay out, lane 1 is a wrong guess, lane 0 lands behind it" % (K - 1),
               lambda m, c, K=K, x=x: all(lane(m, u)["start"] is None for u in range(2, K)) and lane(m, 1)["start"] == SEG and not lane(m, 1)["true"] and lane(m, 0)["landing"][0] == x)
        c.need("the stitching thread walks %d sequences in one go: %s" % (n, "declined" if extra else "done"),
               lambda m, c, n=n, extra=extra: m[0]["stitched"] == 1 and m[0]["rescue"] == min(n, S.RESCUE) + extra and m[0]["gave_up"] == bool(extra))
        yield c


def _mixed():
    for tag, bck in (("plain", False), ("block_checksums", True)):
        c = Case("mixed/" + tag, bsid=5, bck=bck, aim="256 KiB blocks: compressed, stored, compressed with a planted pair, stored, a short last block" + ("; block checksums" if bck else ""))
        c.blk(); c.full()
        c.fr.stored(c.lit(c.fr.bs))
        c.blk(); c.plain_to(2 * SEG); c.fill_to(2 * SEG + 1023); c.long(mark="t1"); c.long(mark="t2"); c.full()
        c.fr.stored(c.lit(c.fr.bs))
        c.blk(); c.plain_to(SEG); c.fill_to(SEG + 16); c.long(mark="u1"); c.long(mark="u2"); c.finish(SEG + SCAN + 2049 + 300)
        c.need("three compressed blocks, none declined, the planted tokens are starts",
               lambda m, c: len(m) == 3 and not any(x["gave_up"] for x in m) and m[1]["lanes"][2]["start"] == c.at["t1"] and m[2]["lanes"][1]["start"] == c.at["u1"] and m[1]["lanes"][2]["true"] and m[2]["lanes"][1]["true"])
        yield c


FAMILIES = [("lanes", _lanes), ("pairs", _pairs), ("cand", _cand), ("decoy", _decoy), ("over", _over), ("notes", _notes), ("exits", _exits), ("rescue", _rescue), ("mixed", _mixed)]
MEMBERS = dict(lanes=7, pairs=9, cand=9, decoy=6, over=6, notes=12, exits=9, rescue=2, mixed=2)
_CORPUS = None


def corpus():
    """[(case, frame bytes, decoded bytes)], built once per process."""
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = []
        for _, gen in FAMILIES:
            for c in gen():
                assert c.b is None, (c.name, "a block was left open")
                _CORPUS.append((c, c.fr.bytes(), bytes(c.fr.out)))
    return _CORPUS


def verdicts(c, fb, density="case"):
    """The model on every compressed block of a frame: a list, in block order.  density: "case" = the case's words, or None."""
    dens = c.density if density == "case" else density
    return [S.model(fb[off:off + w], dens) for off, w in payloads(fb) if not w >> 31]
