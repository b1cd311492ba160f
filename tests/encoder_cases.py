"""Inputs that force an LZ4 encoder's parse, planted on the thresholds of the format and of this library's passes (test helper,
not a test module; numpy only).

A case is a background of random bytes in which no 4-byte window occurs twice - so no encoder finds a match in it - with repeats
("plants") of known length M and distance D copied in behind literal runs of known length L.  The only matches an encoder can then
write are the plants, cut where the writer rules of the block format cut them (lz4_writer_rules.py): `Case.expected(bs)` is that list.
Every case is rebuilt from its name alone (numpy's PCG64 seeded by the name's CRC32, plus the attempt number when a draw had to be
repeated because a window did occur twice or a plant could be extended by a byte).

What makes a plant findable by every finder (liblz4's, csrc/encode_solo.cuh, csrc/encode_hc.cuh):
  - liblz4 and the deterministic finder index only the positions they probe, and probe at a stride that grows by one with every 64
    misses.  Both index every one of a block's first 64 positions, and every literal position behind a match of under 192 bytes.
    So a short plant (M < 64) lies within 64 bytes behind a "primer" (a 40-byte match) and copies from the block's first 64 bytes -
    the "anchor" - or from the two bytes that end the primer (the position both finders index behind every match);
  - behind a long literal run a plant is M >= 8192 with its source at the case's start: some probe lands on an indexed source
    position, and the backward extension returns the match's start;
  - the lanes of one probe step of the deterministic finder do not see each other's insertions: a source never lies in the
    literal run directly in front of its plant, except where a case says so;
  - a 64 KiB chunk that is not a block's first seeds its table from the 64 KiB in front: every 4th position, the last KiB densely.
    Later entries replace earlier ones, so sources in other chunks are either in that last KiB or long and under ~32 KiB back.
Cases of 4 MiB and more skip the window check and are not held to a whole parse ("forced" is False): the GPU encoders that are
functions of their input must still write every plant as planted, and a frame of about planted_frame_size().

Families (the name's first word): len end lit mlen off carry raw link dense - see the functions below.
"""
from __future__ import annotations

import zlib

import numpy as np

B64, B256, B4M = 1 << 16, 1 << 18, 1 << 22
CHUNK = 1 << 16
FRAMINGS = {                                                # name -> block size id, linked, block checksums, content checksum
    "i64": dict(bsid=4, linked=False, bck=False, cck=False),
    "l64": dict(bsid=4, linked=True, bck=False, cck=False),
    "l256": dict(bsid=5, linked=True, bck=True, cck=False),
    "i4m": dict(bsid=7, linked=False, bck=False, cck=True),
}
BS = {"i64": B64, "l64": B64, "l256": B256, "i4m": B4M}
LIT_T = (15, 270, 525, 16080, 16335)                        # literal-run lengths with 1, 2, 3, 64, 65 length bytes (first of each)
MLEN_T = (19, 274, 529, 15829)                              # match lengths with 1, 2, 3, 63 length bytes ... 15829: the first with 64
LONG = 8192                                                 # a plant every finder finds behind any literal run
FAR = 30000                                                 # ... and from up to 65535 back, through a sparsely seeded table
A_HELD = 4096                                               # the shared finder (timing-dependent) is held to plants of at least this


def windows(a: np.ndarray) -> np.ndarray:
    """Every 4-byte window of a uint8 array as a uint32."""
    a = a.astype(np.uint32)
    return a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)


def unique_stream(rng, n: int) -> np.ndarray:
    """n random bytes in which no 4-byte window occurs twice (the later of two equal windows gets a new first byte, until none is left)."""
    out = rng.integers(0, 256, n, dtype=np.uint8)
    while n >= 5:
        w = windows(out)
        order = np.argsort(w, kind="stable")
        sw = w[order]
        dup = order[1:][sw[1:] == sw[:-1]]
        if len(dup) == 0: break
        out[dup] = rng.integers(0, 256, len(dup), dtype=np.uint8)
    return out


def table_slots(d: np.ndarray):
    """Per 4-byte window of d: its slot in liblz4's two tables (4-byte hash to 13 bits; 5-byte hash to 12 bits) and in
    csrc/encode_solo.cuh's (15/16 of 4096 slots).  Three uint64 arrays."""
    w = windows(d).astype(np.uint64)
    fib = (w * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    five = (w | (np.append(d[4:], 0).astype(np.uint64) << np.uint64(32))) << np.uint64(24)
    return fib >> np.uint64(19), (five * np.uint64(889523592379)) >> np.uint64(52), ((fib >> np.uint64(20)) * np.uint64(15)) >> np.uint64(4)


class _Build:
    """A case's bytes: literals from a stream of fresh bytes, plants copied from what is already there."""

    def __init__(self, stream, seed: int = 0):
        self.d = bytearray()
        self.seed = seed                                    # the case name's CRC32: for what a recipe draws besides bytes
        self.stream, self.at = stream, 0                    # stream None: the counting pass (zeros)
        self.plants, self.ghosts = [], []                   # (pos, M, D); ghosts: repeats no encoder may use (out of reach)
        self.free = bytearray()                             # per byte: 1 for a literal

    @property
    def pos(self) -> int:
        return len(self.d)

    def lit(self, n: int) -> int:
        at = self.pos
        if n:
            self.d += bytes(n) if self.stream is None else self.stream[self.at:self.at + n].tobytes()
            self.free += b"\1" * n
            self.at += n
        return at

    def rep(self, M: int, D: int, ghost: bool = False) -> int:
        at = self.pos
        assert 0 < D <= at and M > 0, (M, D, at)
        if D >= M: self.d += self.d[at - D:at - D + M]
        else: self.d += (bytes(self.d[at - D:]) * (M // D + 1))[:M]
        self.free += bytes(M)
        (self.ghosts if ghost else self.plants).append((at, M, D))
        return at

    def rep_from(self, M: int, src: int, ghost: bool = False) -> int:
        return self.rep(M, self.pos - src, ghost)

    def raw(self, b: bytes):
        self.d += b
        self.free += bytes(len(b))


class Case:
    def __init__(self, name, recipe, framings, forced=True):
        self.name, self.fam, self.recipe, self.framings, self.forced = name, name.split("/")[0], recipe, tuple(framings), forced
        self._built = None

    def build(self):
        """(data, plants, ghosts): plants and ghosts are lists of (position, M, D)."""
        if self._built is not None: return self._built
        seed = zlib.crc32(self.name.encode())
        count = _Build(None, seed)
        self.recipe(count)
        checked = self.forced and count.pos < B4M
        for attempt in range(16):
            rng = np.random.default_rng(seed + attempt)
            b = _Build(unique_stream(rng, count.at) if checked else rng.integers(0, 256, count.at, dtype=np.uint8), seed)
            self.recipe(b)
            d = np.frombuffer(bytes(b.d), np.uint8).copy()
            if not checked: break
            # mend: a free literal that takes part in a flaw gets a new value, the plants are copied again, until nothing is left
            free = np.frombuffer(bytes(b.free), np.uint8).astype(bool)
            for _ in range(40):
                flaws = self.flaws(d, b.plants, b.ghosts)
                if not flaws: break
                at = [max([p for p in where if free[p]], default=-1) for _, where in flaws]
                if min(at) < 0: break                         # a flaw no free literal touches: another draw
                d[at] = rng.integers(0, 256, len(at), dtype=np.uint8)
                for pos, M, D in sorted(b.plants + b.ghosts):
                    if D >= M: d[pos:pos + M] = d[pos - D:pos - D + M]
                    else: d[pos:pos + M] = np.resize(d[pos - D:pos], M)
            if not self.flaws(d, b.plants, b.ghosts): break
        else:
            raise AssertionError("%s: no valid draw" % self.name)
        out = (d.tobytes(), b.plants, b.ghosts)
        if len(out[0]) < (1 << 20): self._built = out
        return out

    def flaws(self, d: np.ndarray, plants, ghosts) -> list:
        """What build() mends and rejects a draw for: _flaws, here; a subclass may judge its cases by more (dict_encoder_cases.py)."""
        return _flaws(d, plants, ghosts)

    @property
    def data(self) -> bytes:
        return self.build()[0]

    def expected(self, bs: int) -> list:
        """The plants as a writer may use them in blocks of bs bytes: (position, M, D, L), L counted from the end of the match in
        front or from the block's start.  A plant that starts after blen - 12 is not written, one that runs past blen - 5 is cut there.
        A block whose payload would then be no smaller than the block is stored: its plants are not written at all."""
        data, plants, _ = self.build()
        ext = lambda v: (v - 15) // 255 + 1 if v >= 15 else 0
        out, prev, size = [], 0, {}
        for pos, M, D in plants:
            b0 = pos // bs * bs
            bend = min(b0 + bs, len(data))
            M = min(M, bend - 5 - pos)
            if bend - b0 < 13 or pos > bend - 12 or M < 4: continue
            L = pos - max(prev, b0)
            out.append((pos, M, D, L))
            prev = pos + M
            size[b0] = size.get(b0, 0) + 1 + ext(L) + L + 2 + ext(M - 4)
            size[b0, "end"] = prev
        for b0 in [k for k in size if isinstance(k, int)]:
            bend = min(b0 + bs, len(data))
            fin = bend - size[b0, "end"]
            if size[b0] + 1 + ext(fin) + fin >= bend - b0: out = [r for r in out if r[0] // bs * bs != b0]
        return out


def planted_frame_size(case: Case, fr: str) -> int:
    """The bytes of the frame that holds exactly the planted parse of `case` in framing `fr` (blocks that would not shrink: stored)."""
    f, bs, n = FRAMINGS[fr], BS[fr], len(case.data)
    ext = lambda v: (v - 15) // 255 + 1 if v >= 15 else 0
    total = 7 + 4 + 4 * int(f["cck"])
    want = case.expected(bs)
    for b0 in range(0, n, bs):
        blen = min(bs, n - b0)
        mine = [r for r in want if b0 <= r[0] < b0 + bs]
        end = mine[-1][0] + mine[-1][1] if mine else b0
        pay = sum(1 + ext(L) + L + 2 + ext(M - 4) for _, M, _, L in mine) + 1 + ext(b0 + blen - end) + (b0 + blen - end)
        total += 4 + (pay if mine and pay < blen else blen) + 4 * int(f["bck"])
    return total


def _flaws(d: np.ndarray, plants, ghosts) -> list:
    """[(what, byte positions that take part)] - what keeps a case from being what it says:
      - a plant that is no copy, or could be a byte longer at either end;
      - a 4-byte window that occurs twice outside the plants; a short plant whose first window occurs before it anywhere but at its
        source (the search that keeps the nearest of equal candidates would take that one);
      - a short plant (M < 64) is found by one or two probes, each through one table entry: no position indexed between the source
        and the probe may share that entry's slot, in any of table_slots()'s three tables.  (Of a match's positions the finders
        index the last but one only.)"""
    bad = []
    inside = np.zeros(max(len(d) - 3, 0), bool)                # windows that lie wholly inside a plant: copies by construction
    unindexed = np.zeros(len(d), bool)
    for k, (pos, M, D) in enumerate(list(plants) + list(ghosts)):
        if not np.array_equal(d[pos:pos + M], d[pos - D:pos - D + M]): bad.append(("plant %d is no copy" % k, []))
        if pos + M < len(d) and d[pos + M] == d[pos + M - D]: bad.append(("plant %d extends forwards" % k, [pos + M]))
        if pos - D > 0 and d[pos - 1] == d[pos - D - 1]: bad.append(("plant %d extends backwards" % k, [pos - 1, pos - D - 1]))
        if M >= 4: inside[pos:pos + M - 3] = True
        unindexed[pos:pos + M] = True
        unindexed[pos + M - 2] = False
    if len(d) >= 4:
        at = np.flatnonzero(~inside)
        w = windows(d)[at]
        order = np.argsort(w, kind="stable")
        sw = w[order]
        for p in at[order[1:][sw[1:] == sw[:-1]]].tolist(): bad.append(("the window at %d occurs before, outside the plants" % p, list(range(p, p + 4))))
    if any(M < 64 for _, M, _ in plants) and len(d) >= 5:
        allw = windows(d)
        for k, (pos, M, D) in enumerate(plants):             # (inside other plants too: a long overlapping copy holds its source many times)
            if 4 <= M < 64 and D >= 4:
                twice = np.flatnonzero(allw[:pos] == allw[pos])
                for q in twice[twice != pos - D].tolist(): bad.append(("plant %d: its first window also occurs at %d" % (k, q), list(range(q, q + 4))))
        slots = table_slots(d)
        for k, (pos, M, D) in enumerate(plants):
            if M >= 64: continue
            for j in range(min(4, M - 3)):
                s, probe = pos - D + j, pos + j
                if probe >= len(slots[0]): break
                between = np.arange(s + 1, probe)
                between = between[~unindexed[between]]
                for t, h in enumerate(slots):
                    for q in between[h[between] == h[s]].tolist():
                        bad.append(("plant %d: position %d takes its source's table slot before the probe" % (k, q), list(range(q, min(q + (5 if t == 1 else 4), len(d))))))
    return bad


def problems(data: bytes, plants, ghosts) -> list[str]:
    return [what for what, _ in _flaws(np.frombuffer(data, np.uint8), plants, ghosts)]


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
def _anchor(b) -> int:
    """A block's first 64 bytes: every finder indexes all of them.  [0, 24): sources of short plants; [24, 64): the primer's."""
    return b.lit(64)


def _primer(b, base: int):
    b.rep_from(40, base + 24)


def _filler(b, n: int):
    """n bytes that cost a literal run of 64 and one long match (64 fresh bytes repeated)."""
    assert n >= 72, n
    b.lit(64); b.rep(n - 64, 64)


def _end_block(b, blen: int, mode: str, v: int, after: int = 0):
    """A block (from a block's start) of blen bytes that ends in a 24-byte plant and v literals (mode k), or in a plant that starts
    v bytes before the end and runs to it (mode s).  `after`: literals behind it, in the same block (blen is then a chunk's end)."""
    base = _anchor(b)
    R = 24 if mode == "k" else v
    k = v if mode == "k" else 0
    tail = 5 + 40 + 3 + R + k
    _filler(b, blen - 64 - tail)
    b.lit(5); _primer(b, base); b.lit(3)
    b.rep_from(R, base)
    b.lit(k + after)


def _sparse_pair(b, L: int, M: int = LONG):
    """Source A, source B, a copy of A, L literals, a copy of B: the literal run L `behind another match`."""
    a = b.lit(M); b.lit(8); s = b.lit(M)
    b.rep_from(M, a); b.lit(L); b.rep_from(M, s)


# ---------------------------------------------------------------------------------------------------------------------
def _len_cases():
    def periodic(n): return lambda b: b.raw((b"abcab" * (n // 5 + 1))[:n])
    def rand(n): return lambda b: b.lit(n)
    for n in range(34):
        yield Case("len/periodic/%d" % n, periodic(n), ("i64", "l64", "l256", "i4m"), False)
        yield Case("len/random/%d" % n, rand(n), ("i64", "l64", "l256", "i4m"), False)
    for fr, B in (("i64", B64), ("l64", B64), ("l256", B256), ("i4m", B4M)):
        for n in range(B - 13, B + 14):
            yield Case("len/periodic/%s/%d" % (fr, n), periodic(n), (fr,), False)
            yield Case("len/random/%s/%d" % (fr, n), rand(n), (fr,), False)


def _end_cases():
    import lz4_grammar
    ks = sorted(set(lz4_grammar.END_K) | set(range(14)))
    for mode, vals in (("k", ks), ("s", range(4, 17))):
        for v in vals:
            yield Case("end/short/%s%d" % (mode, v), (lambda m, x: lambda b: _end_block(b, 700 + x, m, x))(mode, v), ("i64", "l256", "i4m"))
            yield Case("end/full/%s%d" % (mode, v), (lambda m, x: lambda b: _end_block(b, B64, m, x))(mode, v), ("i64", "l64"))
            def behind(b, m=mode, x=v):
                b.lit(B64); _end_block(b, 900 + x, m, x)
            yield Case("end/behind_full/%s%d" % (mode, v), behind, ("i64", "l64"))
    # a 64 KiB chunk's end inside a bigger block: no rule applies there
    for k in ks:
        yield Case("end/seam/k%d" % k, (lambda x: lambda b: _end_block(b, CHUNK, "k", x, after=1000))(k), ("l256", "i4m"))
    for s in range(4, 17):
        def seam(b, s=s):
            base = b.lit(64)                                  # [8, 36) and [36, 64): two primers
            _filler(b, CHUNK - s - 447)
            b.lit(5); b.rep_from(28, base + 8); b.lit(3)
            src = b.lit(216 + 100)                            # behind a short match: its first 64 positions are all indexed
            b.rep_from(28, base + 36); b.lit(3)
            assert b.pos == CHUNK - s, b.pos
            b.rep_from(s + 200, src); b.lit(300)              # continues across the seam, from the KiB in front of it
        yield Case("end/seam/s%d" % s, seam, ("l256", "i4m"))


LITS = (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526, 16079, 16080, 16081, 16334, 16335)


def _lit_cases():
    small = ("i64", "l64", "l256", "i4m")
    for L in LITS:
        if L:                                                 # as a block's first sequence: L literals, then they repeat
            yield Case("lit/first/L%d" % L, (lambda L: lambda b: (b.lit(L), b.rep(max(LONG, 2 * L) if L < LONG else LONG, L), b.lit(20)))(L), small)
        yield Case("lit/mid/L%d" % L, (lambda L: lambda b: (_sparse_pair(b, L), b.lit(20)))(L), small)
    def over_chunk(b):                                        # a run longer than a chunk, in front of a match 20000 back
        b.lit(CHUNK + 1064); b.rep(LONG, 20000); b.lit(20)
    yield Case("lit/first/L66600", over_chunk, ("l256", "i4m"))
    for k in (5, 6, 14, 15, 16, 269, 270, 16080):             # the block's final run
        def final(b, k=k):
            a = b.lit(LONG); b.lit(300); b.rep_from(LONG, a); b.lit(k)
        yield Case("lit/final/%d" % k, final, small)
    for L in (0, 1, 15):                                      # a linked block's first sequence, from the block in front
        def linked(b, L=L):
            b.lit(B64 - FAR - 100); a = b.lit(FAR); b.lit(100)
            assert b.pos == B64
            b.lit(L); b.rep_from(FAR, a); b.lit(20)
        yield Case("lit/first_linked/L%d" % L, linked, ("l64",))


MLENS = (4, 5, 18, 19, 20, 273, 274, 275, 528, 529, 15828, 15829, 15830)


def _short_plant(b, L: int, M: int, tail: int = 20):
    """anchor, 20 literals, primer, L literals, M bytes of the anchor, tail."""
    base = _anchor(b)
    b.lit(20); _primer(b, base); b.lit(L); b.rep_from(M, base); b.lit(tail)


def _mlen_cases():
    small = ("i64", "l64", "l256", "i4m")
    for M in MLENS:
        if M <= 24:
            yield Case("mlen/M%d" % M, (lambda M: lambda b: _short_plant(b, 3, M))(M), small)
        else:                                                 # source at the case's start, 200 literals, the plant
            yield Case("mlen/M%d" % M, (lambda M: lambda b: (b.lit(M + 200), b.rep(M, M + 200), b.lit(20)))(M), small)
    # overlapping: D < M.  Short ones copy from the primer's last two bytes on (D = L + 2); D = 1 is a run of the literal in front.
    for M in (19, 20, 273, 529, 15829):
        for D in (1, 2, 3, 7):
            def ovl(b, M=M, D=D):
                base = _anchor(b)
                b.lit(20); _primer(b, base); b.lit(1 if D == 1 else D - 2); b.rep(M, D); b.lit(20)
            yield Case("mlen/ovl/M%d/D%d" % (M, D), ovl, small)
    big = ("l256", "i4m")
    yield Case("mlen/chunk", lambda b: (b.lit(1000), b.rep(CHUNK - 1000 + CHUNK + 500, 1000), b.lit(20)), big)
    yield Case("mlen/M70000", lambda b: (b.lit(5000), b.rep(70000, 5000), b.lit(20)), big)
    yield Case("mlen/M200000", lambda b: (b.lit(5000), b.rep(200000, 5000), b.lit(20)), big)


def _off_cases():
    small = ("i64", "l64", "l256", "i4m")
    for D in (1, 2, 3, 4, 7, 8, 15, 16, 63, 64, 65):
        for M in (20, 300):
            def near(b, M=M, D=D):
                base = _anchor(b)
                b.lit(20); _primer(b, base); b.lit(1 if D == 1 else D - 2); b.rep(M, D); b.lit(20)
            yield Case("off/D%d/M%d" % (D, M), near, small)
    for D in (65534, 65535, 65536):
        def far(b, D=D):
            b.lit(100 + D); b.rep(FAR, D, ghost=D > 65535); b.lit(20)        # (99 bytes into the second chunk: a match starts no later than 4 bytes before a chunk's end)
        yield Case("off/D%d" % D, far, ("l256", "i4m"))


THRESH = (15, 270, 525, 16080)


def _carry_chunk0(b, t: int, block_at: int = 0):
    """A block's first chunk: a match that ends t bytes before the chunk's end, and in front of it 8 KiB for a later plant to copy.
    -> that source's position."""
    a = b.lit(LONG)
    _filler(b, CHUNK - t - 3 * LONG)
    s = b.lit(LONG)
    b.rep_from(LONG, a); b.lit(t)
    assert b.pos - block_at == CHUNK
    return s


def _carry_cases():
    both = ("l256", "i4m")
    for T in THRESH:
        for tag, f, t in (("f_below", T - 1, 1), ("f_on", T, 255), ("f_on_no_cross", T, 1), ("t_alone", 0, T)):
            def adj(b, f=f, t=t):
                s = _carry_chunk0(b, t)
                b.lit(f); b.rep_from(LONG, s); b.lit(20)
            yield Case("carry/adjacent/T%d/%s" % (T, tag), adj, both)
    # chunks without a record in between: their 65536 literals each join the carry
    for n, frs in ((1, both), (2, both), (62, ("i4m",))):
        tot = 15 + 255 * ((n * CHUNK - 15) // 255 + 1)        # the first threshold the carry can reach
        room = tot - n * CHUNK
        for tag, f, t in (("f_below", room - 1, 1), ("f_on", room, 255), ("t_alone", 0, room)):
            def gap(b, n=n, f=f, t=t):
                _carry_chunk0(b, t)
                b.lit(n * CHUNK - 20000); s = b.lit(20000)
                b.lit(f); b.rep_from(LONG if n < 2 else 19000, s); b.lit(20)      # (behind two chunks liblz4's stride outruns 8 KiB)
            yield Case("carry/gap%d/%s" % (n, tag), gap, frs, forced=n < 62)
    for fin in (15, 270, 16080, CHUNK + 14, 2 * CHUNK + 13):  # the block's only match in its first chunk: the final run collects the rest
        def first_only(b, fin=fin):
            t = fin % CHUNK if fin > CHUNK else min(fin, 7)
            _carry_chunk0(b, t); b.lit(fin - t)
        yield Case("carry/first_only/final%d" % fin, first_only, both)
    for n in (1, 3):                                          # the block's only match in its last chunk
        for f in (14, 15, 269, 270):
            def last_only(b, n=n, f=f):
                b.lit(n * CHUNK - 20000); s = b.lit(20000)
                b.lit(f); b.rep_from(LONG if n < 2 else 19000, s); b.lit(20)
            yield Case("carry/last_only/gap%d/f%d" % (n, f), last_only, both)
    for c in (1, 2, 3):                                       # a last chunk of under 4 bytes: the plant runs to the block's end
        for t in (0, 15 - c, 270 - c):
            def tiny(b, c=c, t=t):
                a = b.lit(LONG)
                _filler(b, CHUNK - 2 * LONG - t)
                if t: b.rep_from(LONG, a); b.lit(t + c)
                else: b.rep_from(LONG + c, a)
            yield Case("carry/tiny_last/c%d/t%d" % (c, t), tiny, both)


def _raw_cases():
    # anchor, 20 literals, primer (40), 3 literals, M bytes of the anchor, K literals with 35 length bytes: the payload is
    # blen + 35 - 31 - M bytes (tokens, offsets and length bytes against the 40 + M bytes the matches save)
    K = 15 + 255 * 34
    for M, delta in ((6, -2), (5, -1), (4, 0)):
        yield Case("raw/short/%+d" % delta, (lambda M: lambda b: _short_plant(b, 3, M, K))(M), ("i64", "l256", "i4m"))
        def behind(b, M=M):
            b.lit(B64); _short_plant(b, 3, M, K)
        yield Case("raw/behind_full/%+d" % delta, behind, ("i64", "l64"))


def _link_cases():
    def straddle(b):
        b.lit(B64 - 4096); a = b.lit(4096 + 4096); b.lit(300); b.rep_from(LONG, a); b.lit(20)
    yield Case("link/straddle", straddle, ("l64",))
    for D in (65535, 65536):
        def reach(b, D=D):
            b.lit(B64 + 20); b.rep(FAR, D, ghost=D > 65535); b.lit(20)
        yield Case("link/reach/D%d" % D, reach, ("l64",))
    def third(b):
        b.lit(2 * B64); b.rep(FAR, 2 * B64, ghost=True); b.lit(20)
    yield Case("link/block3_repeats_block1", third, ("l64",))


def _dense(b, nseq: int, specials=()):
    """nseq sequences of 8..20 bytes: 4..8 literals and a 5..12-byte copy of what begins at an earlier literal run.  Each run is
    copied from once, its first bytes are literals behind a short match (every finder indexed them), and a match lies between it
    and its copy (see the module's notes).  Behind a match of 192 bytes and more - where the deterministic finder probes every 4th
    position, and whose source, the runs in front, is now there twice - the next copies come from runs set aside for that.
    `specials`: {sequence number: (L, M)} puts thresholds among them."""
    base = _anchor(b)
    b.lit(20); _primer(b, base)
    rng = np.random.default_rng(b.seed)
    runs, aside = [base, base + 12], []                       # where copies may start: the anchor, then literal runs behind short matches
    prev_long = False
    last_end = b.pos                                          # where the last match ends
    specials = dict(specials)
    planted = 0
    for i in range(nseq):
        L, M = specials.get(i, (int(rng.integers(4, 9)), int(rng.integers(5, 13))))
        was_long = prev_long
        if was_long and M < 8: M = 8
        at = b.lit(L)
        turn = i % 4 == 1                                     # every 4th run is set aside; once 4 are there, the oldest is used in its turn
        src = None
        if M >= LONG: src = at                                # (behind a long run: the run itself repeats)
        elif not turn and runs and runs[0] < last_end: src = runs.pop(0)
        elif aside and aside[0] < last_end and (not turn or len(aside) >= 4): src = aside.pop(0)
        if src is not None:
            b.rep_from(M, src)
            last_end = b.pos
            planted += 1
        prev_long = src is not None and M >= 192
        if src is not None:                                   # (a run whose first bytes the copy holds is there twice: no source any more)
            hi = b.pos if b.pos - M - src < M else src + M
            runs, aside = [r for r in runs if not src < r <= hi - 4], [r for r in aside if not src < r <= hi - 4]
        if L >= 4 and not was_long and not prev_long: (aside if turn else runs).append(at)
    assert planted >= nseq - 4 * sum(M >= 192 for _, M in specials.values()) - 12, (planted, nseq)
    b.lit(20)


def _dense_cases():
    small = ("i64", "l256", "i4m")
    yield Case("dense/plain", lambda b: _dense(b, 300), small)
    sp = {20: (14, 18), 40: (15, 19), 60: (16, 20), 80: (269, 12), 100: (270, 12), 120: (271, 12), 140: (6, 273), 160: (6, 274),
          180: (524, 12), 200: (525, 12), 220: (6, 528), 240: (6, 529)}
    yield Case("dense/thresholds", lambda b: _dense(b, 300, sp), small)
    # the emit pass's switch: records * 192 <= chunk bytes takes the record walk, one byte less the 64-at-once path
    for path, short in (("walk", 0), ("batch", 1)):
        def switch(b, short=short):
            _dense(b, 19)
            b.lit(192 * len(b.plants) - short - b.pos)        # (every plant is a record)
        yield Case("dense/switch/%s" % path, switch, small)
    def big(b):                                               # lengths of 64 and more length bytes on the 64-at-once path (its put_ext loop;
                                                              # the scalar `vbig` branch belongs to the record walk, which lit/ and mlen/ take)
        _dense(b, 420, {200: (16080, LONG), 300: (6, 15829)})
    yield Case("dense/vbig", big, small)


def cases() -> list:
    out = []
    for gen in (_len_cases, _end_cases, _lit_cases, _mlen_cases, _off_cases, _carry_cases, _raw_cases, _link_cases, _dense_cases):
        out += list(gen())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CORPUS = None


def corpus() -> list:
    global _CORPUS
    if _CORPUS is None: _CORPUS = cases()
    return _CORPUS


def in_framing(fr: str) -> list:
    return [c for c in corpus() if fr in c.framings]


# ---------------------------------------------------------------------------------------------------------------------
# What a frame's parse reached: the thresholds above as labels, counted from any encoder's frames.
L_MARKS = frozenset(LITS) | {CHUNK + 1064}
FINAL_MARKS = frozenset((5, 6, 14, 15, 16, 269, 270, 16080))
M_MARKS = frozenset(MLENS) | {70000, 200000, 2 * CHUNK - 500}
D_MARKS = frozenset((1, 2, 3, 4, 7, 8, 15, 16, 63, 64, 65, 65534, 65535))
SHAPES = (["L=%d" % v for v in sorted(L_MARKS)] + ["final=%d" % v for v in sorted(FINAL_MARKS)] + ["M=%d" % v for v in sorted(M_MARKS)] +
          ["D=%d" % v for v in sorted(D_MARKS)] + ["carry/%d" % t for t in THRESH] + ["carry-chunks/%d" % k for k in (1, 2)] +
          ["start=blen-12", "end=blen-5", "stored", "vbig-L", "vbig-M", "emit-walk", "emit-batch"])


def _ext(v: int) -> int:
    return (v - 15) // 255 + 1 if v >= 15 else 0


def shapes(P, merged) -> set:
    """The labels of SHAPES a frame shows.  P: lz4_index.Parsed; merged: lz4_writer_rules.matches(frame, P).
      L= final= M= D=   a literal run / final run / match (neighbours merged) / offset of exactly that size
      carry/T           a literal run that starts in one 64 KiB chunk of a block and ends in a later one, whose share in the last
                        chunk has fewer length bytes than the whole and the whole at least T: pass S's correction term at work
      carry-chunks/k    a literal run that holds k whole chunks (k = 2: two or more) and has more length bytes than its share in
                        the chunk where its match is found: the carry of chunks without a record
      start=blen-12, end=blen-5, stored      a match on the writer rules' limits; a block stored raw
      vbig-L, vbig-M    a sequence with more than 64 literal-length / match-length bytes (pass E2's scalar branch)
      emit-walk, emit-batch      a chunk with records * 192 <= its bytes, and one with more (pass E2's two paths)"""
    out = set()
    for pos, ml, off, lit in merged.tolist():
        if lit in L_MARKS: out.add("L=%d" % lit)
        if ml in M_MARKS: out.add("M=%d" % ml)
        if off in D_MARKS: out.add("D=%d" % off)
    for B in P.blocks:
        if B["stored"]:
            out.add("stored"); continue
        S, blen = B["seqs"], B["out_len"]
        if int(S[-1, 2]) in FINAL_MARKS: out.add("final=%d" % int(S[-1, 2]))
        M = S[:-1]
        if len(M) == 0: continue
        start = M[:, 1] + M[:, 2]
        if np.any(start == blen - 12): out.add("start=blen-12")
        if int(start[-1] + M[-1, 3]) == blen - 5: out.add("end=blen-5")
        if np.any(M[:, 2] >= 16080): out.add("vbig-L")
        if np.any(M[:, 3] >= 15829): out.add("vbig-M")
        crosses = np.flatnonzero(M[:, 1] // CHUNK != start // CHUNK)
        for k in crosses.tolist():
            L = int(M[k, 2]); f = int(start[k]) % CHUNK
            for t in THRESH:
                if L >= t and _ext(f) < _ext(L) and f < t: out.add("carry/%d" % t)
            whole = int(start[k]) // CHUNK - (int(M[k, 1]) + CHUNK - 1) // CHUNK
            if whole >= 1 and _ext(f) < _ext(L): out.add("carry-chunks/%d" % min(whole, 2))
        nrec = np.bincount(start // CHUNK, minlength=(blen + CHUNK - 1) // CHUNK)
        for c, n in enumerate(nrec.tolist()):
            if n: out.add("emit-walk" if n * 192 <= min(CHUNK, blen - c * CHUNK) else "emit-batch")
    return out
