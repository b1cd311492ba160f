"""Inputs for pass E1's forward measurement of a match in rows of dwords (E1_V7 in csrc/encode.cuh; tests/test_gpu_e1_match_rows.py, and
their oracle side in tests/test_e1_match_rows_cpu.py), and a numpy model of that measurement.

Each input is three tiles and a bit (192 KiB + 77 bytes) of random bytes in which no 4-byte window occurs twice, with copies of known
(start, length M, distance D) planted in it - encoder_cases' builder and its checks: every plant is a copy, is followed and preceded by
a byte that differs, and nothing else repeats.  What a plant is there for is in MARKS: (input, what) -> (start, M, D).

How a plant comes to be taken whole, from its first byte, by liblz4's greedy parse and by k_find_matches with one wave parsing (behind a
match's end both probe every position of the next 64 bytes, then every 2nd of the next 128, every 3rd of the next 192, ...; both index
what they probe, and the one position at which they find a match; both extend a match backwards over the literals in front):
  - an input is cells: 32 literals, a plant, 32 literals, a plant, ...  A literal run begins where a match ends, so its first byte is
    probed and indexed by both finders, and the plant behind it is probed at its first byte;
  - a plant copies from the first byte of an earlier literal run that no plant has copied from before (the table then holds one
    position for its first four bytes; should another position have taken that slot, the next probes find the literal run's next
    bytes, and the match is extended back).  Between the plants that are there for something lie "pads", plants like them, that
    only move the next cell to where it has to be;
  - distances 2..5 overlap their own literal run, and the lanes of one probe step do not see each other's entries: those plants lie
    where the stride is their distance (96, 224, 416, 672 bytes behind a match's end), and are found as a run; 255 and 256 copy from
    their own literal run's first bytes;
  - k_find_matches hands out 1 KiB helpings where sequences are long; a helping starts at stride 4, 5, 6, 7 whatever lies in front of
    it, and extends a match no further back than its own first byte.  So no literal run contains a multiple of 1 KiB; a literal
    run of 32 puts its plant on the stride-4 grid; the plants that need strides 1, 2, 3, ... have a match of 64 bytes in front of
    their literal run that begins and ends in their helping; and a plant that crosses a tile's end has the first byte of a literal
    run as the source of its first byte in the next tile;
  - so that the frames are not all matches, each input holds random bytes by the tens of KiB.  The match behind such a stretch is a
    copy of its last 8 KiB: found somewhere inside and extended back (see _Lay.mass);
  - a block's first 8 KiB are 4 KiB of literals and their copy, which leaves a run's first tile sparse.
"""
from __future__ import annotations

import numpy as np

import encoder_cases as ec

KIB = 1 << 10
TILE = 1 << 16
N = 3 * TILE + 77
RUN_ENV = {"LZ4F_MI355X_E1_RUN": "16"}
ONE_WAVE_ENV = {"LZ4F_MI355X_E1_SOLO": "5", "LZ4F_MI355X_E1_RUN": "16"}
# (name, oracle.mkprefs keywords)
FRAMINGS = [("indep64k", dict(bsid=4, indep=1)), ("indep4m", dict(bsid=7, indep=1))]
BLOCK = {"indep64k": 1 << 16, "indep4m": 1 << 22}
LENGTHS = (4, 5, 255, 256, 257, 259, 260, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1535, 1536, 1537, 3 * 768 + 1)   # row and round edges, 2..4 rows
PHASES = tuple((a, b) for a in range(4) for b in range(4))             # (start & 3, (start - D) & 3), at M = 513
RUN_D = {1: 32, 2: 96, 3: 224, 4: 416, 5: 672, 255: 255, 256: 256}     # distance -> the literal run in front (see above)
FAR_D = (4093, 65535)
M_PHASE = 513
MARKS = {}                                                             # (input, what) -> (start, M, D); filled when an input is built


def _run_ok(e: int, p0: int) -> bool:
    """A literal run [e, p0) in front of a plant: one helping probes all of it, from e on."""
    return e % KIB != 0 and e // KIB == (p0 + 3) // KIB


def _end_ok(end: int) -> bool:
    return _run_ok(end, end + 32)


class _Lay:
    """Cells on an encoder_cases._Build."""

    def __init__(self, b, name: str):
        self.b, self.name, self.pool = b, name, []

    def lit(self, g: int, keep: bool = True) -> int:
        e = self.b.lit(g)
        if keep: self.pool.append(e)
        return e

    def opening(self, stock: int = 30):
        """A block's first 8 KiB and 100 bytes: 4 KiB of literals and their copy - a run's first tile counts no more than that one match in
        the 4 KiB it is judged by, and is searched as sparse.  Then a stock of literal runs to copy from, 32 bytes each, between copies
        of 64 bytes from the block's 21st, 22nd, ... byte: every finder probes a block's first 64 positions one by one and indexes them,
        and finds the 4 KiB copy within its first 20 bytes (the position where it does is indexed for the second time, there)."""
        assert stock <= 30
        at = self.b.pos
        self.lit(4 * KIB, keep=False)
        self.b.rep(4 * KIB + 100, 4 * KIB)
        for k in range(stock):
            assert _end_ok(self.b.pos)
            self.lit(32)
            M = 64
            while not _end_ok(self.b.pos + M): M += 1
            self.b.rep_from(M, at + 20 + k)

    def take(self, p0: int, want=lambda e: True, far: int = 65000, newest: bool = False) -> int:
        """The first byte of the oldest (newest) literal run that nothing has copied from, within reach of a plant at p0."""
        for k in (range(len(self.pool) - 1, -1, -1) if newest else range(len(self.pool))):
            e = self.pool[k]
            if 200 < p0 - e <= far and want(e): return self.pool.pop(k)
        raise AssertionError("%s: no source left for a plant at %d" % (self.name, p0))

    def pad(self, M: int):
        """A plant that is there to fill M bytes."""
        assert M >= 64, (self.name, M, self.b.pos)
        self.b.rep_from(M, self.take(self.b.pos))

    def goto(self, e: int):
        """From a plant's end to a literal run that starts at e: 32 literals and a pad, as often as it takes."""
        while True:
            assert _end_ok(self.b.pos), (self.name, self.b.pos)
            self.lit(32)
            rest = e - self.b.pos
            assert rest >= 64, (self.name, e, self.b.pos)
            if rest <= 3000: self.pad(rest); return
            L = 2000
            while not (_end_ok(self.b.pos + L) and e - (self.b.pos + L) >= 32 + 64): L += 1
            self.pad(L)

    def mass(self, p0: int, M: int = 8 * KIB):
        """Random bytes up to p0 - what keeps the frame from being all matches - and the match that ends them: a copy of their last M
        bytes.  Behind a literal run this long both finders probe every n-th position only and have indexed as few, so this one is
        found somewhere inside and extended back: by liblz4 as far as it goes, by k_find_matches to its helping's first byte at most -
        p0 lies 100 bytes into a helping, where that one's stride is 4, and M is a multiple of the helping's size, so that the first
        position probed at or behind p0 has a source that was probed too."""
        assert p0 % KIB == 100 and M % KIB == 0 and p0 - self.b.pos >= M + 2 * KIB, (self.name, p0, self.b.pos)
        self.lit(p0 - self.b.pos)
        self.b.rep(M, M)

    def spot(self, M: int, g: int = 32, phase: int | None = None, at: int = 0, cut: bool = False, lead: bool = False, fit=lambda p0: True) -> int:
        """The first place at or behind `at` where a plant of M bytes behind a literal run of g can start."""
        g0 = g + (96 if lead else 0)
        p0 = max(at, self.b.pos + 32 + 64 + g0)
        while not ((phase is None or p0 & 3 == phase) and _run_ok(p0 - g0, p0) and (cut or _end_ok(p0 + M)) and fit(p0)): p0 += 1
        return p0

    def cell(self, what, M: int, p0: int, src: int | None = None, g: int = 32, D: int | None = None, want=lambda e: True, newest: bool = False,
             lead: bool = False):
        """A literal run of g and a plant of M bytes at p0: at distance D, or copied from src, or (neither given) from the oldest
        literal run left that `want` accepts.  -> where the plant starts (its literal run: g in front).
        lead: 32 literals and a match of 64 in front of the literal run, in the same helping - the match in front then ends in the
        helping that found it, which goes on from there at stride 1, 2, 3, ...  (a helping that begins behind a match that reached into
        it starts at stride 4, as every helping does)."""
        if lead:
            self.goto(p0 - g - 96)
            self.lit(32)
            self.b.rep_from(64, self.take(self.b.pos))
        else:
            self.goto(p0 - g)
        if src is None and D is None: src = self.take(p0, want, newest=newest)
        self.lit(g, keep=D is None or D > g)                   # (a run that its own plant copies from is no source for another)
        assert self.b.pos == p0
        at = self.b.rep(M, D) if D is not None else self.b.rep_from(M, src)
        if what is not None: MARKS[self.name, what] = (at, M, at - src if D is None else D)
        return at

    def crossing(self, what, end: int, M_a: int, M):
        """A plant that lies across `end` (a tile's), and whose first byte behind it is copied from the first byte of a literal run: the
        source is a literal run, M_a bytes, a literal run, 64 bytes, and the literal run in question.  M: its length, or a function of
        where it starts.  -> where the literal run in front of it starts."""
        def kept(M):                                           # (a cell whose literal run no other plant copies from)
            e = self.cell(None, M, self.spot(M, at=self.b.pos + 96)) - 32
            self.pool.remove(e)
            return e
        sa, sb, sc = kept(M_a), kept(64), kept(64)
        p0 = end - (sc - sa)
        assert _run_ok(p0 - 32, p0) and p0 >= self.b.pos + 32 + 64 + 32, (self.name, what, p0, self.b.pos)
        self.cell(what, M if isinstance(M, int) else M(p0), p0, src=sa)
        return p0 - 32


def _main(b):
    """192 KiB + 77 as ONE block: every length, phase and distance; the ring's wrap; a tile's end; the block's end far into a match."""
    y = _Lay(b, "main")
    y.opening()
    y.mass(30 * KIB + 100)
    for k, M in enumerate(LENGTHS[1:]):                        # (M = 4: a block of 64 KiB and more is searched by five bytes - see _blocks)
        y.cell("M=%d" % M, M, y.spot(M, phase=k & 3))
    # a plant across the first tile's end; and a plant in the second tile whose source lies across that end (offset 65536 of the input
    # is where the ring of a run of tiles wraps)
    ew = y.crossing("tile 1 opens inside", TILE, 100, 700)
    y.pool.remove(ew)
    assert ew < TILE < ew + M_PHASE
    y.cell("source across the wrap", M_PHASE, y.spot(M_PHASE, at=b.pos + 1000), src=ew)
    far = y.pool[-1]                                           # (kept for the plant 65535 bytes on)
    y.pool.remove(far)
    for D, g in RUN_D.items():
        y.cell("D=%d" % D, M_PHASE, y.spot(M_PHASE, g=g, lead=True), g=g, D=D, lead=True)
    y.mass(100 * KIB + 100)
    for a, s in PHASES:
        if not any(e & 3 == s and b.pos - e > 100 for e in y.pool):        # (a literal run at that phase to copy from: 32 in front of a cell at it)
            y.cell(None, 100, y.spot(100, phase=s))
        y.cell("phase %d %d" % (a, s), M_PHASE, y.spot(M_PHASE, phase=a), want=lambda e: e & 3 == s)
    D = FAR_D[0]
    src = next(e for e in y.pool if e + D >= b.pos + 800 and _run_ok(e + D - 32, e + D) and _end_ok(e + D + M_PHASE))
    y.pool.remove(src)
    y.cell("D=%d" % D, M_PHASE, src + D, src=src)
    # the second tile's end inside a plant of 1025 bytes: its first round of rows is cut there
    y.crossing("into the tile's end", 2 * TILE, 100, 1025)
    D = FAR_D[1]
    p0 = far + D
    assert p0 >= b.pos + 128 and _run_ok(p0 - 32, p0) and _end_ok(p0 + M_PHASE), (far, b.pos)
    y.cell("D=%d" % D, M_PHASE, p0, src=far)
    y.mass(178 * KIB + 100)
    # the block's end, 77 bytes into the fourth tile: a match that the third tile's end cuts in a round of rows behind the first, and
    # whose rest is cut five bytes before the block's end
    y.crossing("into the block's end", 3 * TILE, 1500, lambda p0: N - p0)
    assert b.pos == N


def _blocks(b):
    """Three blocks of 64 KiB and one of 77 bytes: M = 4 (blocks under 64 KiB + 11 are searched by four bytes), and each block's end
    inside a match - in its first round of rows, far behind it, and one byte into a round of three rows."""
    for k, M_end in enumerate((300, 2000, 769)):
        y = _Lay(b, "blocks")
        base = k * TILE
        y.opening()
        for _ in range(3):
            y.cell(None, 600, y.spot(600, at=b.pos + 100))
        if k == 0:
            # 4 and 5 bytes: literal run and plant inside one 128-byte slice, the source a few cells back
            for M in (4, 5):
                slice_ok = lambda p0: (p0 - 32) % 128 != 0 and (p0 - 32) // 128 == (p0 + M + 3) // 128
                y.cell("M=%d" % M, M, y.spot(M, at=b.pos + 300, fit=slice_ok), newest=True)      # (no plant in between has copied its source's bytes)
                y.cell(None, 600, y.spot(600, at=b.pos + 200))
        y.mass(base + 53 * KIB + 100)
        p0 = y.spot(M_end, at=base + TILE - M_end, cut=True)
        y.cell("block %d's end" % k, base + TILE - p0, p0)
        assert b.pos == base + TILE
    b.lit(77)


_RECIPES = {"main": (_main, ("indep4m",)), "blocks": (_blocks, ("indep64k",))}
NAMES = tuple(_RECIPES)
CASE_FRAMINGS = {n: fr for n, (_, fr) in _RECIPES.items()}
_CASES = {}


def _slot_flaws(d: np.ndarray, plants, free: np.ndarray) -> list:
    """A plant is found through ONE table entry, its source's: no literal between the two (every literal is probed, and indexed) may
    share that entry's slot, in any of encoder_cases.table_slots()'s tables.  [(what, byte positions that take part)]"""
    bad = []
    slots = ec.table_slots(d)
    lits = np.flatnonzero(free[:len(slots[0])])
    for k, (pos, M, D) in enumerate(plants):
        s = pos - D
        if s >= len(slots[0]): continue
        between = lits[np.searchsorted(lits, s + 1):np.searchsorted(lits, pos)]
        for t, h in enumerate(slots):
            for q in between[h[between] == h[s]].tolist():
                bad.append(("plant %d: position %d takes its source's table slot" % (k, q), list(range(q, min(q + (5 if t == 1 else 4), len(d))))))
    return bad


def case(name: str) -> ec.Case:
    """The input as an encoder_cases.Case (its data, its plants, what a writer may use of them), drawn and mended as Case.build() does,
    with the table slots of ALL plants looked at, not only the short ones'."""
    if name in _CASES: return _CASES[name]
    import zlib
    recipe = _RECIPES[name][0]
    c = ec.Case("rows/" + name, recipe, ())
    seed = zlib.crc32(c.name.encode())
    count = ec._Build(None, seed)
    recipe(count)
    for attempt in range(16):
        rng = np.random.default_rng(seed + attempt)
        b = ec._Build(ec.unique_stream(rng, count.at), seed)
        recipe(b)
        d = np.frombuffer(bytes(b.d), np.uint8).copy()
        free = np.frombuffer(bytes(b.free), np.uint8).astype(bool)
        flaws = None
        for _ in range(60):
            flaws = ec._flaws(d, b.plants, []) + _slot_flaws(d, b.plants, free)
            if not flaws: break
            at = [max([p for p in where if free[p]], default=-1) for _, where in flaws]
            if min(at) < 0: break                              # a flaw no free literal touches: another draw
            d[at] = rng.integers(0, 256, len(at), dtype=np.uint8)
            for pos, M, D in sorted(b.plants):
                if D >= M: d[pos:pos + M] = d[pos - D:pos - D + M]
                else: d[pos:pos + M] = np.resize(d[pos - D:pos], M)
        if not flaws: break
    else:
        raise AssertionError("%s: no valid draw" % c.name)
    c._built = (d.tobytes(), b.plants, [])
    _CASES[name] = c
    return c


def data(name: str) -> bytes:
    return case(name).data


def expected(name: str, framing: str) -> list:
    """(start, M, D, literals in front) of every plant as a writer of blocks of that size may use it: cut five bytes before a block's end."""
    return case(name).expected(BLOCK[framing])


def marks(name: str) -> dict:
    case(name)
    return {what: v for (n, what), v in MARKS.items() if n == name}


_ORACLE = {}


def oracle_frame(name: str, framing: str) -> bytes:
    """liblz4's frame (the oracle's port) of an input in a framing; made once."""
    import oracle
    if (name, framing) not in _ORACLE:
        _ORACLE[(name, framing)] = oracle.conduit_compress(data(name), oracle.mkprefs(**dict(FRAMINGS)[framing]))
    return _ORACLE[(name, framing)]


# ---------------------------------------------------------------------------------------------------------------------
# the measurement, as the kernel does it
RING = 2 * TILE
RMASK = RING - 1


def ring_of(d: np.ndarray, tile: int) -> np.ndarray:
    """The kernel's ring while it searches tile `tile` of a run that began at the input's first byte: input position p at ring offset
    (p + 64 KiB) mod 128 KiB - this tile, the one in front and whatever older bytes the rest still holds - and its first 16 bytes again
    behind its end."""
    ring = np.zeros(RING + 16, np.uint8)
    for t in range(max(tile - 2, 0), tile + 1):
        part = d[t * TILE:(t + 1) * TILE]
        at = ((t + 1) * TILE) & RMASK
        ring[at:at + len(part)] = part
    ring[RING:] = ring[:16]
    return ring


def _alignbyte(hi: np.ndarray, lo: np.ndarray, k: int) -> np.ndarray:
    return (((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(8 * k)).astype(np.uint32)


def rows_forward(ring: np.ndarray, mp: int, d: int, cap: int, rows: int) -> int:
    """How far the bytes at ring position mp and those d in front of them agree, at most cap: rounds of `rows` rows; lane i of row r
    reads the two dwords at the dword at or below base + 256 r + 4 i (masked to the ring) and picks its four bytes by the base's byte
    phase; the first row with a difference, its first lane, that lane's first differing byte."""
    dw = ring[:RING + 16].view("<u4")
    lane = np.arange(64, dtype=np.int64)
    fw = 0
    while True:
        base = mp + fw
        n = rows * 256
        for r in range(rows):
            a = base + 256 * r + 4 * lane
            i1, i2 = ((a & RMASK) & ~3) >> 2, (((a - d) & RMASK) & ~3) >> 2
            x = _alignbyte(dw[i1 + 1], dw[i1], base & 3) ^ _alignbyte(dw[i2 + 1], dw[i2], (base - d) & 3)
            diff = np.flatnonzero(x)
            if len(diff):
                f = int(diff[0]); xv = int(x[f])
                n = 256 * r + 4 * f + ((xv & -xv).bit_length() - 1 >> 3)
                break
        fw += n
        if n == rows * 256 and fw < cap: continue
        return min(fw, cap)


def bytes_forward(ring: np.ndarray, mp: int, d: int, cap: int) -> int:
    i = (mp + np.arange(cap, dtype=np.int64)) & RMASK
    diff = np.flatnonzero(ring[i] != ring[(i - d) & RMASK])
    return int(diff[0]) if len(diff) else cap
