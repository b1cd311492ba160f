"""Planted inputs for the dictionary encoders of the batch call, on the edges where only a dictionary finder can be wrong (test
helper, not a test module; numpy + the oracle only).

encoder_cases.py forces an encoder's parse by planting repeats in a background without any; dict_cases.py has the frame walk and
the dictionary model.  This module puts the two together: a case belongs to one dictionary, and its input is drawn and mended by
encoder_cases.Case.build itself over the concatenation [dictionary | input] with the dictionary's bytes frozen, so the flaw checks
hold across the seam: no 4-byte window occurs twice in dictionary and input together, a plant cannot be extended by a byte, and no
indexed position hides a short plant's source in a finder's table.  (The concatenation holds the whole dictionary, also the front
of one longer than 64 KiB that no encoder may use: a repeat of it is a ghost.)

Plants are (position in the input, M, distance); a distance larger than the position: the source lies in the dictionary.  A plant
is kept as the natural copy it is in the concatenation, and `expected(case, framing)` turns it into what an encoder that keeps the
seam policy (csrc/encode_solo.cuh, csrc/encode_hc.cuh: a match's source lies on one side of the seam) may write in a framing:
  - the dictionary sits in front of every block of an independent frame, so a copy of dictionary bytes p.. at offset o of a later
    block is a plant at distance o + D - p there - and a ghost in a linked frame, where the dictionary sits in front of the first
    byte only and 64 KiB of input lie between;
  - a plant whose source runs across the seam is two: the dictionary's part, then the input's first bytes at the same distance
    (a part of under 4 bytes: literals);
  - what is left is cut at the blocks' ends by encoder_cases.Case.expected.
Ghosts are repeats no encoder may use: 65536 and more back, or from the front of a dictionary that does not count.

Families (DCase.fam): reach/far reach/ghost reach/first reach/last seam/cross seam/back mpos0 block2 chunk/last_reach chunk/second
pick - see cases().  tests/golden/dict_planted.json (tools/mint_dict_planted.py) records what liblz4 1.9.3 writes of every case
with an LZ4F_CDict at levels 0 and 9; a (case, framing) is `forced` where its level-9 parse is the planted one.
"""
from __future__ import annotations

import json
import os
import zlib

import numpy as np

import dict_cases as dc
import encoder_cases as ec
from lz4_grammar import Frame, lz4_seq

KB64 = dc.KB64
MINMATCH = 4
DENSE = 1024                                                  # csrc/encode_solo.cuh's SOLO_SEED_DENSE: the history's last KiB is seeded position by position
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict_planted.json")
DICT_LEN = {"k4": 4, "k7": 7, "k64": 64, "k1k": 1024, "k64k-1": 65535, "k64k": 65536, "k70k": 70000}
FRAMINGS = ("i64", "l64", "l256")
SEAM_FAMILIES = ("seam/cross", "seam/back")                   # compared sequence by sequence; the others with neighbours merged
MUST_BE_FORCED = ("reach/far", "reach/ghost", "reach/first", "reach/last", "seam/cross")
FAMILIES = MUST_BE_FORCED + ("seam/back", "mpos0", "block2", "chunk/last_reach", "chunk/second", "pick")

_dicts: dict = {}


def dictionary(name: str) -> bytes:
    """unique_stream bytes seeded from the dictionary's name."""
    if name not in _dicts:
        _dicts[name] = ec.unique_stream(np.random.default_rng(zlib.crc32(("dict/" + name).encode())), DICT_LEN[name]).tobytes()
    return _dicts[name]


def counted(name: str) -> int:
    """The bytes of a dictionary that count: its last 64 KiB at most."""
    return min(DICT_LEN[name], KB64)


class DCase(ec.Case):
    """A case of one dictionary.  The recipe writes the input behind the dictionary's bytes: `b.pos - DL` is a position in the input,
    a source below DL lies in the dictionary (DL: the whole dictionary's length)."""

    def __init__(self, name, fam, dname, recipe, framings=FRAMINGS, allow=()):
        self.dname, self.DL, self.D = dname, DICT_LEN[dname], counted(dname)
        d = dictionary(dname)
        super().__init__(name, lambda b: (b.raw(d), recipe(b, self.DL)), framings)
        self.fam = fam
        self.allow = tuple(allow)                             # (a word of _flaws' verdict, the concatenation's positions it names): flaws a case is about

    def flaws(self, d, plants, ghosts):
        """encoder_cases._flaws over [dictionary | input], less what the case is about and less the table slots an independent
        frame's later block never saw.  The slots that the dictionary's own (frozen) positions take are judged here:
          - a dictionary of more than DENSE bytes fills every slot of a one-entry table many times over, which is why the finders
            with such a table (liblz4's fast one, encode_solo.cuh) are held to the parse for the dictionaries of at most DENSE
            bytes only - a chain search (liblz4's level 9, encode_hc.cuh) loses no source to a later one;
          - a dictionary of at most DENSE bytes is seeded position by position, later ones winning (encode_solo.cuh): a short
            plant is found if the probe at its first byte or the one two bytes on (the stride behind 64 misses is 2) still finds
            its source there - the match's start comes back from the backward extension.  A plant that has neither is a flaw no
            draw mends: the case needs another source."""
        bad = [(what, where) for what, where in ec._flaws(d, plants, ghosts)
               if not any(word in what and tuple(where) == tuple(at) for word, at in self.allow)
               and not ("table slot" in what and (where[0] < self.DL or self._other_block(where[0], plants)))]
        slots = None
        for k, (pos, M, D) in enumerate(plants):              # a plant across the seam: its second part is found through the input's first bytes
            K = pos - D + M - self.DL
            if not (pos - D < self.DL and MINMATCH <= K < 64): continue
            if slots is None:
                slots, unindexed = ec.table_slots(d), np.zeros(len(d), bool)
                for p2, m2, _ in list(plants) + list(ghosts): unindexed[p2:p2 + m2] = True; unindexed[p2 + m2 - 2] = False
            for j in range(min(4, K - 3)):
                between = np.arange(self.DL + j + 1, pos + M - K + j)
                between = between[~unindexed[between]]
                for t, h in enumerate(slots):
                    for q in between[h[between] == h[self.DL + j]].tolist():
                        bad.append(("plant %d: position %d takes the table slot of its second part's source before the probe" % (k, q), list(range(q, min(q + (5 if t == 1 else 4), len(d))))))
        if self.D <= DENSE and self.DL >= MINMATCH:
            solo = ec.table_slots(d[:self.DL])[2]
            for k, (pos, M, D) in enumerate(plants):
                s = pos - D
                if not (M < 64 and s < self.DL and min(M, self.DL - s) >= MINMATCH): continue     # (the dictionary's part of it)
                seen = [j for j in (0, 2) if j <= min(M, self.DL - s) - MINMATCH and not np.any(solo[s + j + 1:] == solo[s + j])]
                if not seen: bad.append(("plant %d: later positions of the dictionary take the table slots of its source's first bytes" % k, []))
        return bad

    def _other_block(self, q: int, plants) -> bool:
        """A position of the input's first 64 KiB, where a short plant of a later block copies the dictionary: _flaws counts it
        between source and probe, but such a plant is planted in independent blocks alone, whose tables never saw it."""
        return any(pos - self.DL >= KB64 and pos - D < self.DL and self.DL <= q < self.DL + KB64 for pos, M, D in plants if M < 64)

    # ---- the input's side ----
    @property
    def data(self) -> bytes:
        return self.build()[0][self.DL:]

    def plants(self) -> list:
        """(position in the input, M, distance) as planted in [dictionary | input]."""
        return [(pos - self.DL, M, D) for pos, M, D in self.build()[1]]

    def expected(self, fr: str) -> list:
        """(position, M, distance, L) rows of the planted parse in framing `fr` (see the module's notes)."""
        inner = ec.Case(self.name, None, (fr,))
        inner._built = (self.data, [r for r, ok in self._placed(fr) if ok], [])
        return inner.expected(ec.BS[fr])

    def ghosts(self, fr: str) -> list:
        """(position, M) of the repeats no encoder may use in framing `fr`: the case's ghosts and the plants out of reach there."""
        return [(pos - self.DL, M) for pos, M, _ in self.build()[2]] + [(x, M) for (x, M, _), ok in self._placed(fr) if not ok]

    def _placed(self, fr: str) -> list:
        """[((position, M, distance in this framing), whether an encoder may use it)]: plants cut at the seam, the distance of a
        dictionary's copy counted from the dictionary in front of its scope."""
        bs, linked, DL = ec.BS[fr], ec.FRAMINGS[fr]["linked"], self.DL
        out = []
        for x, M, dist in self.plants():
            s = x - dist                                      # the source, counted from the seam
            parts = [(x, M)] if s >= 0 or s + M <= 0 else [(x, -s), (x - s, M + s)]
            if len(parts) == 2: assert x + M <= bs, "a plant across the seam stays in the first block"
            for px, pm in parts:
                if pm < MINMATCH: continue
                ps = px - dist
                if ps >= 0:                                   # the input's own bytes
                    ok = dist <= 65535 and (linked or ps >= px // bs * bs)
                    out.append(((px, pm, dist), ok))
                else:
                    scope = 0 if linked else px // bs * bs
                    eff = dist - scope
                    ok = eff <= 65535 and ps + DL >= DL - self.D
                    out.append(((px, pm, eff if ok else dist), ok))
        return out


# ---------------------------------------------------------------------------------------------------------------------
def _upto(b, DL: int, x: int):
    b.lit(DL + x - b.pos)


def _full_block(b, DL: int):
    """The input's first 64 KiB at the price of 64 literals and one match (encoder_cases._filler)."""
    assert b.pos == DL
    ec._filler(b, KB64)


def _payer(b, M: int):
    """Behind a plant of M bytes that alone would not make its block smaller (a match saves M - 3 bytes, the sequence behind it
    costs a token, a literal run of 15 and more a length byte): 64 literals and 100 bytes that repeat them, or every encoder
    stores the block and the plant is never written."""
    if M < 8: ec._filler(b, 164); b.lit(20)


def cases() -> list:
    out = []

    def add(name, fam, dname, recipe, **kw):
        out.append(DCase(name, fam, dname, recipe, **kw))

    big = ("k64k-1", "k64k", "k70k")
    for dn in big:
        for M in (40, 600):
            for x in (1, 100):
                # the farthest source there is, and the same bytes one dictionary byte earlier
                add("reach/far/%s/M%d/x%d" % (dn, M, x), "reach/far", dn, lambda b, DL, M=M, x=x: (_upto(b, DL, x), b.rep(M, 65535), b.lit(20)))
                add("reach/ghost/%s/M%d/x%d" % (dn, M, x), "reach/ghost", dn, lambda b, DL, M=M, x=x: (_upto(b, DL, x), b.rep(M, 65536, ghost=True), b.lit(20)))
    add("reach/ghost/k70k/front", "reach/ghost", "k70k", lambda b, DL: (_upto(b, DL, 100), b.rep_from(40, 100, ghost=True), b.lit(20)))
    for dn in ("k4", "k7", "k64", "k1k"):
        for x in (1, 100):
            add("reach/first/%s/x%d" % (dn, x), "reach/first", dn, lambda b, DL, x=x: (_upto(b, DL, x), b.rep_from(min(DL, 40), 0), b.lit(20), _payer(b, min(DL, 40))))
    for dn in ("k7", "k64", "k1k") + big:
        for M in (4, 5, 40):
            if M > DICT_LEN[dn]: continue
            add("reach/last/%s/M%d" % (dn, M), "reach/last", dn, lambda b, DL, M=M: (_upto(b, DL, 20), b.rep_from(M, DL - M), b.lit(20), _payer(b, M)))
    for dn in ("k64", "k1k", "k64k"):
        for K in (1, 3, 4, 30):
            # d[-40:] and the input's own first K bytes behind it: one copy in [dictionary | input], cut at the seam by expected()
            add("seam/cross/%s/K%d" % (dn, K), "seam/cross", dn, lambda b, DL, K=K: (_upto(b, DL, 50), b.rep_from(40 + K, DL - 40), b.lit(20)))
        # the dictionary's last byte and input[0:40]: the match may not grow backwards into the dictionary
        add("seam/back/%s" % dn, "seam/back", dn, lambda b, DL: (_upto(b, DL, 100), b.rep_from(41, DL - 1), b.lit(20)))
    for dn, p in (("k64", 10), ("k1k", 300), ("k64k", 30000), ("k64k-1", 0)):
        add("mpos0/%s" % dn, "mpos0", dn, lambda b, DL, p=p: (b.rep_from(40, p), b.lit(30)))

    def block2(b, DL):
        _full_block(b, DL); b.lit(100); b.rep_from(40, 500); b.lit(160)
    add("block2/k1k", "block2", "k1k", block2)

    def last_reach(b, DL):
        # ends two bytes before the first chunk's end, 65535 back: 41 bytes in front of the seam
        ec._filler(b, KB64 - 42 - 30); b.lit(30)
        assert b.pos - DL == KB64 - 42
        b.rep(40, 65535); b.lit(2 + 100)
    add("chunk/last_reach/k1k", "chunk/last_reach", "k1k", last_reach)

    def second(b, DL):
        _full_block(b, DL); b.lit(10); b.rep_from(40, 600, ghost=True); b.lit(150)
    # (in 64 KiB independent blocks this is block2's plant; a ghost where the frame is linked - in l256 as a block's second chunk)
    add("chunk/second/k1k", "chunk/second", "k1k", second, framings=("l64", "l256"))

    for dn, p in (("k1k", 200), ("k64k", 40000)):
        def pick(b, DL, p=p):
            b.lit(30); first = b.rep_from(8, p); b.lit(40); b.rep_from(60, p); b.lit(20)
            return first
        first = DICT_LEN[dn] + 30
        add("pick/%s" % dn, "pick", dn, pick, allow=[("first window also occurs", range(first, first + 4))])
    names = [c.name for c in out]
    assert len(set(names)) == len(names) and {c.fam for c in out} == set(FAMILIES)
    return out


_CORPUS = None


def corpus() -> list:
    global _CORPUS
    if _CORPUS is None: _CORPUS = cases()
    return _CORPUS


def of_dictionary(dname: str, fr: str) -> list:
    return [c for c in corpus() if c.dname == dname and fr in c.framings]


def pairs() -> list:
    return [(c, fr) for c in corpus() for fr in c.framings]


# ---------------------------------------------------------------------------------------------------------------------
# parses: a frame's (or the fixture's) sequences per block -> rows to compare with DCase.expected
def frame_seqs(frame: bytes) -> list:
    """Per block its raw sequences [(literals, match length, offset)], the last with match length 0; None for a stored block."""
    return [None if stored else [tuple(s) for s in dc.sequences(frame[at:at + n])] for stored, at, n in dc.walk(frame)["blocks"]]


def block_lengths(seqs: list, n: int, bs: int) -> list:
    return [min(bs, n - b * bs) for b in range(len(seqs))]


def rows(seqs: list, n: int, bs: int, merge: bool) -> list:
    """(position in the content, M, distance, literals in front) of every match; merge: a match that begins where the one before
    ends, at the same offset and not at a block's start, is its continuation - lz4_writer_rules.matches' rule."""
    out = []
    for b, S in enumerate(seqs):
        if S is None: continue
        pos = b * bs
        for lit, ml, off in S:
            pos += lit
            if ml == 0: break
            if merge and lit == 0 and out and out[-1][2] == off and out[-1][0] + out[-1][1] == pos and pos > b * bs: out[-1][1] += ml
            else: out.append([pos, ml, off, lit])
            pos += ml
    return [tuple(r) for r in out]


def parse_of(case: DCase, fr: str, seqs: list) -> list:
    return rows(seqs, len(case.data), ec.BS[fr], case.fam not in SEAM_FAMILIES)


def straddlers(seqs: list, n: int, bs: int, linked: bool) -> list:
    """The raw sequences whose source range [pos - off, pos - off + min(mlen, off)) holds a dictionary byte and an input byte: an
    overlapping match is judged by where its reads begin and by the first `off` bytes, what lies behind is its own output."""
    bad = []
    for pos, ml, off, _ in rows(seqs, n, bs, False):
        s = pos - (0 if linked else pos // bs * bs) - off     # counted from the seam in front of the match's scope
        if s < 0 < s + min(ml, off): bad.append((pos, ml, off))
    return bad


def literal_everywhere(seqs: list, n: int, bs: int, spans) -> bool:
    """No match of the parse covers a byte of `spans` [(position, length)]."""
    return not any(p < x + m and x < p + ml for p, ml, _, _ in rows(seqs, n, bs, False) for x, m in spans)


def planted_frame(case: DCase, fr: str) -> bytes:
    """The frame that holds exactly the planted parse (a block that would not shrink: stored), written with lz4_grammar."""
    f, bs, data = ec.FRAMINGS[fr], ec.BS[fr], case.data
    frame = Frame(f["bsid"], linked=f["linked"], bck=f["bck"], cck=f["cck"])
    want = case.expected(fr)
    for b0 in range(0, len(data), bs):
        blen = min(bs, len(data) - b0)
        at, payload = b0, b""
        for x, M, dist, L in [r for r in want if b0 <= r[0] < b0 + bs]:
            assert x - at == L
            payload += lz4_seq(data[at:x], M, dist)
            at = x + M
        payload += lz4_seq(data[at:b0 + blen], 0, 0)
        if at > b0 and len(payload) < blen: frame.raw_block(payload, blen)
        else: frame.stored(data[b0:b0 + blen])
    frame.out = bytearray(data)
    return frame.bytes()


# ---- the fixture ----
def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def is_forced(fx: dict, case: DCase, fr: str) -> bool:
    """liblz4's level 9 wrote the planted parse."""
    got = [None if S is None else [tuple(s) for s in S] for S in fx["cases"][case.name][fr]["seqs9"]]
    return parse_of(case, fr, got) == case.expected(fr)


def check_sha(fx: dict):
    for dname in DICT_LEN:
        assert dc.sha(dictionary(dname)) == fx["dicts"][dname]["sha256"], "dictionary %s is not the one the fixture was minted from" % dname
    assert set(fx["cases"]) == {c.name for c in corpus()}
    for c in corpus():
        assert dc.sha(c.data) == fx["cases"][c.name]["sha256"], "input %s is not the one the fixture was minted from" % c.name
