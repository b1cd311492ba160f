"""Inputs on which the hash-chain encoder of levels 3-12 has to DECIDE: which of several candidates wins, when the chain walk gives
up, when the lazy parse moves on, how far a match is pulled back, and where the finder's own seams lie (test helper, not a test
module; numpy, and the library's datagen for synthetic text).

A case does not say what is expected: tests/hc_model.py does.  A case only makes the outcome hinge on the decision it is named
for, and tests/test_hc_model_cpu.py checks on the model alone that it does.  Every case is rebuilt from its name (numpy's PCG64
seeded by the name's CRC32); a draw in which a chance hash collision takes the decision away is drawn again (`decides`).

Building blocks.  A background of bytes in which no 4-byte window occurs twice (encoder_cases.unique_stream), and on it:
  target      the bytes at the event's position p: a key and a body, in front of them a byte of their own
  candidate   a copy of the target's first `length` bytes, then a byte that differs; the byte in front differs too (unless the
              case is about extending backwards)
  decoy       4 bytes with the 13-bit hash of a given window and other bytes: a position that costs the walk an attempt and
              matches nothing.  With the attempts set to 1 (LZ4F_MI355X_HC_ATTEMPTS) a decoy behind a source hides it from one
              position: that is how a match is found at p and not at p-1, so that it has to be extended backwards.

Framings: i64 (64 KiB independent blocks), i256 (256 KiB independent: chunks with 64 KiB of their own block in front), l64 (64 KiB
linked).  A case's `levels` are run as they are; `attempts` (where not None) is the environment switch the engine is made with;
`dictionary` goes through the prepared HC dictionary of the batch call.  meta["p"]: the event's position in the input.
"""
from __future__ import annotations

import zlib

import numpy as np

from encoder_cases import unique_stream
import hc_model as hm

CHUNK = 1 << 16
FRAMINGS = {"i64": dict(bsid=4, bs=1 << 16, linked=False), "i256": dict(bsid=5, bs=1 << 18, linked=False),
            "l64": dict(bsid=4, bs=1 << 16, linked=True)}
ALL = ("i64", "i256", "l64")
HC_T, LANES, RING = 960, 64, 65536 + 2 * 960
STRIDE = LANES - 2                                           # the parse's window moves on by 62 positions where nothing is found
MAX_LEN = 4 * CHUNK + 777


def hash13(b) -> int:
    v = int.from_bytes(bytes(b[:4]), "little")
    return ((v * 2654435761) & 0xFFFFFFFF) >> 19


class Lay:
    """A case's bytes: a unique background of n bytes, and what is put on it at chosen positions."""

    def __init__(self, rng, n: int):
        self.rng, self.d = rng, unique_stream(rng, n).copy()
        self.meta = {}

    def rnd(self, n: int) -> bytes:
        return bytes(self.rng.integers(0, 256, n, dtype=np.uint8))

    def put(self, at: int, b) -> int:
        b = bytes(b)
        assert 0 <= at and at + len(b) <= len(self.d), (at, len(b), len(self.d))
        self.d[at:at + len(b)] = np.frombuffer(b, np.uint8)
        return at + len(b)

    def get(self, at: int, n: int) -> bytes:
        return self.d[at:at + n].tobytes()

    def target(self, p: int, body: bytes, pre: int = 0x11) -> int:
        """body at p, behind the byte `pre`, and a byte behind it that the candidates do not have."""
        self.put(p - 1, bytes([pre]))
        return self.put(p, body)

    def cand(self, at: int, body: bytes, length: int, pre: int = 0x11 ^ 0xA5) -> int:
        """body[:length] at `at`, then a byte that is not body[length]; in front a byte that is not the target's."""
        if at > 0 and pre is not None: self.put(at - 1, bytes([pre]))
        nxt = body[length] ^ 0x5A if length < len(body) else None
        return self.put(at, body[:length] + (bytes([nxt]) if nxt is not None else b""))

    def decoys(self, at: int, windows) -> int:
        """One decoy per 4-byte window, from `at` on: 4 bytes of the same hash and another value."""
        for w4 in windows:
            h = hash13(w4)
            while True:
                v = self.rng.integers(0, 256, (4096, 4), dtype=np.uint8)
                x = v.astype(np.uint32)
                hv = (((x[:, 0] | (x[:, 1] << 8) | (x[:, 2] << 16) | (x[:, 3] << 24)).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)
                k = np.flatnonzero(hv == h)
                k = [i for i in k.tolist() if v[i].tobytes() != bytes(w4)]
                if k: break
            at = self.put(at, v[k[0]].tobytes())
        return at

    def fill(self, at: int, src: int, n: int = 600) -> int:
        """A copy of n background bytes: what makes a block of literals worth compressing, so that its parse is written."""
        return self.put(at, self.get(src, n))

    def bytes(self) -> bytes:
        return self.d.tobytes()


class Case:
    def __init__(self, name, recipe, framings=ALL, levels=(3, 9), attempts=None, dictionary=None, decides=None):
        self.name, self.fam, self.recipe, self.framings, self.levels = name, name.split("/")[0], recipe, tuple(framings), tuple(levels)
        self.attempts, self.dict_recipe, self.decides = attempts, dictionary, decides
        self._built = None

    def build(self):
        """(data, dictionary or None, meta)"""
        if self._built is None:
            seed = zlib.crc32(self.name.encode())
            for draw in range(12):
                rng = np.random.default_rng(seed + draw)
                self._models = {}
                d = self.dict_recipe(rng) if self.dict_recipe else None
                out = self.recipe(rng, d) if self.dict_recipe else self.recipe(rng)
                data, meta = out if isinstance(out, tuple) else (out, {})
                self._built = (bytes(data), d, meta)
                if self.decides is None or self.decides(self): break
            else:
                self._built = None                           # (kept only when a draw is accepted)
                raise AssertionError("%s: no draw decides" % self.name)
            assert len(self._built[0]) <= MAX_LEN, self.name
        return self._built

    @property
    def data(self) -> bytes: return self.build()[0]

    @property
    def dictionary(self): return self.build()[1]

    @property
    def meta(self) -> dict: return self.build()[2]

    def model(self, fr: str) -> "hm.Model":
        """The case's model in a framing (kept: its searches are shared by every parse of it)."""
        if not hasattr(self, "_models"): self._models = {}
        if fr not in self._models:
            f = FRAMINGS[fr]
            self._models[fr] = hm.Model(self.data, f["bs"], f["linked"], self.dictionary or b"")
        return self._models[fr]

    def parse(self, fr: str, level: int, **how) -> "hm.Parse":
        if self.attempts is not None: how.setdefault("attempts", self.attempts)
        return self.model(fr).parse(level, **how)


def _same(a: "hm.Parse", b: "hm.Parse") -> bool:
    return [B["seqs"] for B in a.blocks] == [B["seqs"] for B in b.blocks]


# ---------------------------------------------------------------------------------------------------------------------
# conditions a draw has to meet (test_hc_model_cpu.py checks them again, on every case)
def attempts_decide(c: Case) -> bool:
    k, fr = c.meta["k"], c.framings[0]
    if k < 2: return True                                    # (the longest is the nearest: any walk finds it)
    P = [c.model(fr).parse(9, attempts=a) for a in (k - 1, k, k + 1)]
    return not (_same(P[0], P[1]) and _same(P[1], P[2]))


def lazy_decides(c: Case) -> bool:
    fr = c.framings[0]
    if "moves" in c.meta:                                    # a staircase: at every level the parse stands on p first, takes every
        if not event_taken(c): return False                  # step, and decides again after at least one reload on the way
        for lvl in c.levels:
            a, z = hm.level_params(lvl)
            e = c.model(fr).windows[0][2].schedule(a, z).get(c.meta["p"] + c.meta["moves"])
            if e is None or e["first_w0"] + e["first"] != c.meta["p"] or e["reloads"] < 1: return False
    return _same(c.parse(fr, 9, lazy=1), c.parse(fr, 9, lazy=2)) != c.meta["lazy_differs"]


def back_decides(c: Case) -> bool:
    p = c.meta["p"]
    for fr in c.framings:
        P = c.parse(fr, 9)
        if _same(P, c.parse(fr, 9, back=False)) == c.meta["back_differs"]: return False
        if [p - r[0] for r in P.rows.tolist() if r[0] <= p < r[0] + r[1]] != [c.meta["pull"]]: return False
        if not any(ev[0] + c0 - win.cs == p for _, c0, _, _, evs, win in P.chunks for ev in evs): return False      # found AT p
    return True


def on_its_lane(c: Case) -> bool:
    """seam/*/laneR: the parse first stands on the event in lane R of a window of full width (R = 62, 63: the look-ahead lanes,
    so lane R - 62 of the window loaded next), at every level of the case; a staircase that begins in lanes 59-61 is decided
    again after a reload."""
    if not event_taken(c): return False
    r, p = int(c.name.split("lane")[1]), c.meta["p"]
    for fr in c.framings:
        for lvl in c.levels:
            a, z = hm.level_params(lvl)
            S = c.model(fr).windows[0][2].schedule(a, z)
            e = S.get(p + c.meta.get("moves", 0))
            if e is None or not e["full"] or e["first_w0"] + e["first"] != p: return False
            if e["first_w0"] != LANE0 + (LANE_K + r // STRIDE) * STRIDE or e["first"] != r % STRIDE: return False
            if "moves" in c.meta and (e["reloads"] >= 1) != (r in (59, 60, 61)): return False
    return True


def event_taken(c: Case) -> bool:
    """The parse takes a match at (or, after lazy moves, behind) the event's position, in every framing and level of the case."""
    p = c.meta["p"]
    for fr in c.framings:
        for lvl in c.levels:
            P = c.parse(fr, lvl)
            rows = P.rows
            if not any(r[0] <= p + c.meta.get("moves", 0) < r[0] + r[1] for r in rows.tolist()): return False
            if "moves" in c.meta and not any(r[0] == p + c.meta["moves"] for r in rows.tolist()): return False    # every step is taken
    return True


def raw_decides(c: Case) -> bool:
    """One block is stored with a payload of its length or a byte more, the other is not, with a byte to spare."""
    B = c.parse(c.framings[0], 9).blocks
    return sorted((b["size"] - b["blen"]) for b in B) == [-1, 0] or sorted((b["size"] - b["blen"]) for b in B) == [-1, 1]


def costs_decide(c: Case) -> bool:
    """With 2 attempts the 30 bytes in the dictionary are not reached, with 3 they are."""
    fr = c.framings[0]
    two, three = c.parse(fr, 9, attempts=2), c.parse(fr, 9, attempts=3)
    return not _same(two, three) and any(src < win.seam for _, _, _, _, ev, win in three.chunks for _, _, src in ev)


def dict_decides(c: Case) -> bool:
    fr = c.framings[0]
    if not c.meta.get("dict_used", True): return True
    P = c.parse(fr, c.levels[0])
    f = FRAMINGS[fr]
    plain = hm.Model(c.data, f["bs"], f["linked"]).parse(c.levels[0], attempts=c.attempts)
    in_dict = any(src < win.seam for _, _, _, _, ev, win in P.chunks for _, _, src in ev)
    return in_dict and not _same(P, plain)


# ---------------------------------------------------------------------------------------------------------------------
def _pick(L: Lay, p: int, cands, tlen: int = None, body: bytes = None):
    """The target at p and candidates [(position, length)]: copies of the target's first `length` bytes."""
    tlen = tlen or max(n for _, n in cands) + 8
    body = body or L.rnd(tlen + 1)
    for at, n in cands: L.cand(at, body, n)
    L.target(p, body[:tlen])
    L.meta["p"] = p
    return body


def _lazy(L: Lay, p: int, src: int, a: int, b: int, ahead: int = 1):
    """A match of a bytes at p and one of b bytes at p + ahead, from two sources (from `src` on).  -> the next free position"""
    body = L.rnd(ahead + b + 9)
    at = L.cand(src + 1, body, a) + 2
    at = L.put(at, bytes([body[ahead - 1] ^ 0xA5]))
    at = L.put(at, body[ahead:ahead + b] + bytes([body[ahead + b] ^ 0x5A])) + 2
    L.target(p, body[:ahead + b + 4])
    L.meta["p"] = p
    return at


def _stairs(L: Lay, p: int, src: int, steps: int, a: int = 6):
    """Position p + i has a match of a + i bytes, i = 0..steps: the one-ahead parse moves `steps` times."""
    body = L.rnd(steps + a + steps + 9)
    at = src + 1
    for i in range(steps + 1):
        if i: at = L.put(at, bytes([body[i - 1] ^ 0xA5]))
        at = L.put(at, body[i:i + a + i] + bytes([body[i + a + i] ^ 0x5A])) + 1
    L.target(p, body[:steps + a + steps + 4])
    L.meta.update(p=p, moves=steps)
    return at


def _pick_cases():
    def three(which):
        def recipe(rng):
            L = Lay(rng, 3000)
            lens = {"nearest": (10, 20, 30), "middle": (10, 30, 20), "farthest": (30, 20, 10), "equal": (20, 20, 20)}[which]
            _pick(L, 2000, list(zip((300, 700, 1100), lens)), 40)
            return L.bytes(), L.meta
        return recipe
    for which in ("nearest", "middle", "farthest", "equal"):
        yield Case("pick/" + which, three(which), decides=event_taken)

    def both_cap(rng):                                        # both reach 258: the nearer ends the walk, though the farther runs on to 400
        L = Lay(rng, 4000)
        _pick(L, 3000, [(300, 400), (1200, 300)], 420)
        return L.bytes(), L.meta
    yield Case("pick/both_at_the_cap", both_cap, decides=event_taken)


def _chain(L: Lay, p: int, first: int, k: int, short: int = 6, long: int = 40, gap: int = 64):
    """The longest candidate is the k-th on p's chain: k - 1 nearer ones of `short` bytes."""
    cands = [(first, long)] + [(first + gap * (i + 1), short) for i in range(k - 1)]
    _pick(L, p, cands, long + 8)
    L.meta["k"] = k


def _attempts_cases():
    for A, ks in ((1, (1, 2)), (2, (1, 2, 3)), (3, (2, 3, 4)), (5, (4, 5, 6))):
        for k in ks:
            def recipe(rng, k=k):
                L = Lay(rng, 2400)
                _chain(L, 2000, 200, k)
                return L.bytes(), L.meta
            yield Case("attempts/A%d/k%d" % (A, k), recipe, ("i64",), (3, 9), attempts=A, decides=attempts_decide)

    def ladder(rng):
        """A key every 7 bytes; most repeats match 4 bytes, and the repeat in the middle of each gap of the levels' ladder matches
        a byte more than every nearer one."""
        key, body = bytes(rng.integers(0, 256, 4, dtype=np.uint8)), bytes(rng.integers(0, 256, 24, dtype=np.uint8))
        special = {10: 5, 40: 6, 56: 7, 160: 8, 320: 9, 448: 10, 768: 11, 1536: 12, 3072: 13, 6144: 14}
        units = []
        for i in range(8250, 0, -1):                           # i: the unit's place on the chain, 1 the nearest
            n = special.get(i, 4)
            fill = bytes([body[n - 4] ^ (1 + int(rng.integers(0, 255)))]) + bytes(rng.integers(0, 256, 2, dtype=np.uint8))
            units.append(key + body[:n - 4] + fill)
        head = bytes(unique_stream(rng, 64))
        d = head + b"".join(units)
        p = len(d)
        d += key + body + bytes(unique_stream(rng, 200))
        assert p <= 65535 and len(d) < CHUNK
        return d, dict(p=p)

    def ladder_decides(c):
        seen = [c.model("i64").parse(lvl) for lvl in range(3, 13)]
        return all(not _same(seen[i], seen[j]) for i in range(10) for j in range(i))
    yield Case("attempts/ladder", ladder, ("i64",), tuple(range(3, 14)), decides=ladder_decides)


def _lazy_cases():
    def one(a, b, ahead):
        def recipe(rng):
            L = Lay(rng, 3000)
            _lazy(L, 2000, 200, a, b, ahead)
            L.fill(2300, 1200, 500)
            L.meta["lazy_differs"] = ahead == 2 and b > a + 1
            return L.bytes(), L.meta
        return recipe
    yield Case("lazy/next_longer_by_1", one(10, 11, 1), decides=lazy_decides)
    yield Case("lazy/next_equal", one(10, 10, 1), decides=lazy_decides)
    yield Case("lazy/second_longer_by_2", one(10, 12, 2), decides=lazy_decides)
    yield Case("lazy/second_longer_by_1", one(10, 11, 2), decides=lazy_decides)

    def stairs(p, n=8000):
        def recipe(rng):
            L = Lay(rng, n)
            _stairs(L, p, 100, 70)
            L.meta["lazy_differs"] = False
            return L.bytes(), L.meta
        return recipe
    yield Case("lazy/stairs_over_a_reload", stairs(7000), decides=lazy_decides)
    yield Case("lazy/stairs_over_a_batch", stairs(7 * HC_T - 30), decides=lazy_decides)      # positions 6690 .. 6760 over 6720

    def beyond(ahead):
        def recipe(rng):                                      # the block ends so that p = last_start (one ahead) or last_start - 1 (two)
            n = 3000
            L = Lay(rng, n)
            p = n - 12 - (ahead - 1)
            _lazy(L, p, 200, 5, 6 if ahead == 1 else 7, ahead)
            L.fill(1500, 900, 500)
            L.d = L.d[:n]
            L.meta["lazy_differs"] = False
            return L.bytes(), L.meta
        return recipe
    yield Case("lazy/look_ahead_beyond_last_start/1", beyond(1), decides=lazy_decides)
    yield Case("lazy/look_ahead_beyond_last_start/2", beyond(2), decides=lazy_decides)

    def capped(rng):                                          # 258 at p (it runs to 270), and 258 that runs to 299 at p + 1: taken at p
        L = Lay(rng, 4000)
        _lazy(L, 3000, 200, 270, 298, 1)
        L.meta["lazy_differs"] = False
        return L.bytes(), L.meta
    yield Case("lazy/cap_at_p_longer_at_next", capped, decides=lazy_decides)


def _hidden_plant(L: Lay, p: int, src: int, k: int, length: int = 24, decoys_at: int = None):
    """A match of `length` bytes at p whose source is at src, and k equal bytes in front of both.  One decoy per window that begins
    in those k bytes, behind the source: with one attempt per position, none of p-k .. p-1 finds the source."""
    front, body = L.rnd(k), L.rnd(length + 1)
    if src - k > 0: L.put(src - k - 1, b"\x77")
    L.put(src - k, front)
    L.cand(src, body, length, pre=None)
    L.put(p - k - 1, b"\x88")
    L.put(p - k, front + body[:length] + bytes([body[length]]))
    seq = front + body[:3]
    L.decoys(decoys_at if decoys_at is not None else src + length + 8, [seq[i:i + 4] for i in range(k)])
    L.meta["p"] = p


def _back_cases():
    for k in (0, 1, 254, 255, 256):
        def recipe(rng, k=k):
            L = Lay(rng, 4000)
            _hidden_plant(L, 3000, 400, k)
            L.meta.update(back_differs=k > 0, pull=min(k, 255))
            return L.bytes(), L.meta
        yield Case("back/by_%d" % k, recipe, ("i64", "l64"), (3, 9), attempts=1, decides=back_decides)

    def prev_match(rng):                                      # a match ends 10 bytes in front of p; 20 bytes in front of p are the source's
        L = Lay(rng, 4000)
        _hidden_plant(L, 3000, 400, 20)
        lead = L.rnd(10)
        L.put(3000 - 30, lead)                                # [p-30, p-10): ten bytes of its own and the first ten of the front
        L.cand(1500, lead + L.get(3000 - 20, 10), 20)
        L.meta.update(back_differs=True, pull=10)
        return L.bytes(), L.meta
    yield Case("back/clipped_by_the_match_in_front", prev_match, ("i64",), (3, 9), attempts=1, decides=back_decides)

    def chunk_start(rng):                                     # p is 5 bytes into a block's second chunk / a linked frame's second block
        L = Lay(rng, CHUNK + 2000)
        _hidden_plant(L, CHUNK + 5, CHUNK - 600, 20)
        L.fill(CHUNK + 1000, CHUNK + 200); L.fill(6000, 5000)
        L.meta.update(back_differs=True, pull=5)
        return L.bytes(), L.meta
    yield Case("back/clipped_by_the_chunk_start", chunk_start, ("i256", "l64"), (3, 9), attempts=1, decides=back_decides)

    def window_start(rng):                                    # the source is 3 bytes behind the window's first byte, and they are equal too
        L = Lay(rng, 3000)
        _hidden_plant(L, 2000, 3, 3)
        L.fill(2300, 1000, 500)
        L.meta.update(back_differs=True, pull=3)
        return L.bytes(), L.meta
    yield Case("back/clipped_by_the_window_start", window_start, ("i64", "l64"), (3, 9), attempts=1, decides=back_decides)


def _long_cases():
    for n in (257, 258, 259, 258 + 511, 258 + 512, 258 + 513, 258 + 1024):
        def recipe(rng, n=n):
            L = Lay(rng, 2 * n + 1500)
            _pick(L, n + 900, [(300, n)], n + 8)
            return L.bytes(), L.meta
        yield Case("long/%d" % n, recipe, ("i64", "l64"), decides=event_taken)

    def to_block_end(rng):                                    # the data ends inside the copy: cut at block end - 5
        L = Lay(rng, 5000)
        L.put(4000, L.get(300, 1000))
        L.meta["p"] = 4000
        return L.bytes(), L.meta
    yield Case("long/to_block_end", to_block_end, decides=event_taken)

    def over_chunk_end(rng):                                  # cut at a chunk's end (i256: it goes on in the next chunk; i64, l64: block end - 5)
        L = Lay(rng, CHUNK + 3000)
        L.put(CHUNK - 700, L.get(300, 1500))
        L.fill(CHUNK + 2000, CHUNK + 1000)
        L.meta["p"] = CHUNK - 700
        return L.bytes(), L.meta
    yield Case("long/over_a_chunk_end", over_chunk_end, decides=event_taken)

    def to_end_lim(rng):                                      # ... and a whole block behind it: end_lim is the block's, and the chunk's
        L = Lay(rng, 2 * CHUNK)
        L.put(2 * CHUNK - 900, L.get(CHUNK + 300, 900))
        L.fill(6000, 5000)
        L.meta["p"] = 2 * CHUNK - 900
        return L.bytes(), L.meta
    yield Case("long/to_end_lim", to_end_lim, decides=event_taken)

    for name, unit in (("zeros", b"\0"), ("period1", None), ("period2", None), ("period3", None)):
        def recipe(rng, name=name, unit=unit):
            L = Lay(rng, 5000)
            u = unit or L.rnd(int(name[-1]))
            L.put(1000, (u * 3000)[:3000])
            L.meta["p"] = 1000 + len(u)
            return L.bytes(), L.meta
        yield Case("long/overlap/" + name, recipe, ("i64",), decides=event_taken)


# lane cases: a match ends at LANE0 and nothing is found from there to the event, so the parse loads its 64-lane windows at
# LANE0 + 62 k.  The parse also starts afresh at every 960 j - 2 (where the results known in an iteration end): LANE0 and the
# event lie between two of those, 1918 and 2878.
LANE0, LANE_K = 1950, 10
SEAM_P = ([("batch%d" % r, 3 * HC_T + r if r < 2 else 2 * HC_T + r, "i64", None) for r in (0, 1, 958, 959)] +
          [("lane%d" % r, LANE0 + LANE_K * STRIDE + r, "i64", None) for r in (59, 60, 61, 62, 63)] +
          [("p%d" % p, p, "two", None) for p in (65536, 65537)] +
          [("src%d" % q, 66000, "two", q) for q in (65535, 65536, 65537)] +
          [("wrap%+d" % (p - RING), p, "two", None) for p in (RING - 1, RING, RING + 1)] +
          [("batch%d_in_chunk2" % r, 69 * HC_T + r if r < 2 else 68 * HC_T + r, "two", None) for r in (0, 1, 958, 959)] +
          # a block's third chunk / a linked frame's third block: the window begins 64 KiB into the input (positions in the window)
          [("wrap+0_in_chunk3", RING, "three", None), ("batch0_in_chunk3", 71 * HC_T, "three", None),
           ("batch959_in_chunk3", 70 * HC_T + 959, "three", None)])


def _seam_cases():
    for tag, p, where, far in SEAM_P:
        frs = ("i64",) if where == "i64" else ("i256", "l64")
        n = 4200 if where == "i64" else 70400 if where == "two" else 2 * CHUNK + 4900
        if where == "three": p += CHUNK
        lane = tag.startswith("lane")

        def fill(L, n):
            if n == 4200: L.fill(3600, 3000, 500)
            else: L.fill(5000, 4000); L.fill(CHUNK + 3700, 4000)
            if n > 2 * CHUNK: L.fill(2 * CHUNK + 3700, CHUNK + 5000)

        def reset(L):                                         # (a 50-byte match that ends at LANE0: the parse's windows begin at LANE0 + 62 k)
            L.put(LANE0 - 50, L.get(LANE0 - 120, 50))

        def pick(rng, p=p, n=n, lane=lane, far=far):
            L = Lay(rng, n)
            src = p - 1500 if p > 60000 else 300
            if far is None: _pick(L, p, [(src, 12), (src + 100, 24), (src + 200, 12)], 32)
            else: _pick(L, p, [(far - 200, 12), (far, 24), (far + 200, 12)], 32)      # the longest candidate AT 65535, 65536, 65537
            if lane: reset(L)
            fill(L, n)
            L.meta.update(lane0=LANE0 if lane else None, src=far, wp=p - CHUNK if n > 2 * CHUNK else p)
            return L.bytes(), L.meta
        yield Case("seam/pick/" + tag, pick, frs, decides=on_its_lane if lane else event_taken)

        if far is not None: continue

        def lazy(rng, p=p, n=n, lane=lane):
            L = Lay(rng, n)
            _stairs(L, p, p - 1500 if p > 60000 else 300, 3)
            if lane: reset(L)
            fill(L, n)
            L.meta.update(lane0=LANE0 if lane else None, wp=p - CHUNK if n > 2 * CHUNK else p)
            return L.bytes(), L.meta
        yield Case("seam/lazy/" + tag, lazy, frs, decides=on_its_lane if lane else event_taken)

    # the reach: a candidate of 40 bytes exactly 65535 back is found; 65536 back it is not, and a nearer one of 8 bytes wins
    for tag, p in (("batch_first", 71 * HC_T), ("batch_last", 71 * HC_T + HC_T - 1)):
        for D in (65535, 65536):
            def reach(rng, p=p, D=D):
                L = Lay(rng, 70400)
                _pick(L, p, [(p - D, 40), (p - 3000, 8)], 48)
                L.fill(5000, 4000); L.fill(CHUNK + 3700, 4000)
                L.meta["D"] = D
                return L.bytes(), L.meta
            yield Case("seam/reach/%s/D%d" % (tag, D), reach, ("i256", "l64"), decides=event_taken)


def _end_cases():
    yield Case("end/block12", lambda rng: b"abc" * 4, ALL)
    yield Case("end/block13", lambda rng: b"a" * 13, ALL)
    yield Case("end/block13_period4", lambda rng: (b"abcd" * 4)[:13], ALL)
    for c in (1, 2, 3, 4):
        def tiny(rng, c=c):                                   # a repeat that runs to the input's end, c bytes into the next chunk / block
            L = Lay(rng, CHUNK + c)
            L.put(CHUNK - 300, L.get(500, 300 + c))
            return L.bytes(), dict(p=CHUNK - 300)
        yield Case("end/last_chunk_of_%d" % c, tiny, ALL, decides=event_taken)
    for d in (0, 1):
        def start(rng, d=d):                                  # a 7-byte (6-byte) copy that begins at last_start (+ 1) and ends at block end - 5
            n = 3000
            L = Lay(rng, n)
            p = n - 12 + d
            L.cand(300, L.get(p, 7 - d) + b"\0", 7 - d)
            L.fill(1500, 900, 500)
            return L.bytes(), dict(p=p)
        yield Case("end/starts_at_last_start%+d" % d, start, ALL)

    def must_end(rng):                                        # the source goes on for 40 bytes more than the block has
        n = 3000
        L = Lay(rng, n + 40)
        L.put(n - 60, L.get(300, 100))
        return L.bytes()[:n], dict(p=n - 60)
    yield Case("end/must_end_at_block_end_minus_5", must_end, ALL, decides=event_taken)


def _text_cases():
    from lz4_frame_conduit_amd import datagen
    from test_gpu_hc import real_text
    n = 2 * CHUNK + 777
    yield Case("text/real", lambda rng: real_text(n), ALL, (3, 6, 9))
    yield Case("text/synth", lambda rng: datagen.synth_text(n).tobytes(), ALL, (3, 6, 9))
    yield Case("text/real96k", lambda rng: real_text(96 << 10), ("i256", "l64"), (12,))
    yield Case("text/synth96k", lambda rng: datagen.synth_text(96 << 10).tobytes(), ("i256", "l64"), (12,))
    yield Case("text/synth50", lambda rng: datagen.synth50(2 * CHUNK).tobytes(), ALL, (9,))


def _raw_cases():
    # block 1: 64 KiB with one match of M bytes behind 30000 literals - the payload is 65536 - M + 261 + ext(M - 4) bytes;
    # block 2: 100 bytes with one match of m bytes behind 50 literals - the payload is 106 - m bytes
    for tag, M, m in (("first_stored", 262, 7), ("second_stored", 263, 6)):
        def recipe(rng, M=M, m=m):
            L = Lay(rng, CHUNK + 100)
            _pick(L, 30000, [(100, M)], M + 4)
            _pick(L, CHUNK + 50, [(CHUNK + 10, m)], m + 4)
            return L.bytes(), dict(p=30000)
        yield Case("raw/" + tag, recipe, ("i64", "l64"), decides=raw_decides)


def _dict_of(n):
    return lambda rng: bytes(unique_stream(rng, n))


def _dict_cases():
    frs = ("i64", "l64")

    def copies(rng, d):                                       # the dictionary's first and last bytes, and a slice of it, among literals
        L = Lay(rng, 3000)
        k = min(40, len(d))
        L.put(500, d[-k:]); L.put(900, d[:k])
        if len(d) > 300: L.put(1500, d[len(d) // 2:len(d) // 2 + 300])
        L.fill(2200, 1600)
        return L.bytes(), dict(dict_used=len(d) >= 4)
    for n in (3, 4, 5, 1024, CHUNK + 100):
        yield Case("dict/len%d" % n, copies, frs, dictionary=_dict_of(n), decides=dict_decides)

    def over_seam_dict(rng, d):                               # the dictionary's last 20 bytes and the input's first 20: cut at the seam
        L = Lay(rng, 2000)
        L.put(1000, d[-20:] + L.get(0, 20))
        return L.bytes(), {}
    yield Case("dict/over_the_seam/from_the_dictionary", over_seam_dict, frs, dictionary=_dict_of(1024), decides=dict_decides)

    def over_seam_input(rng, d):                              # ... its last 3 bytes only: no position straddles, and the input's match
        L = Lay(rng, 2000)                                    # does not extend backwards below the seam
        L.put(1000, d[-3:] + L.get(0, 20))
        L.put(1500, d[-30:])                                  # (and one that ends at the seam)
        return L.bytes(), {}
    yield Case("dict/back_stops_at_the_seam/input_side", over_seam_input, frs, dictionary=_dict_of(1024), decides=dict_decides)

    def hidden_dict(rng):                                     # 5 bytes, a 24-byte source, and behind them a decoy for each of the 5 windows
        L = Lay(rng, 1024)
        L.decoys(100, [L.get(i, 4) for i in range(5)])
        return L.bytes()

    def dict_first_byte(rng, d):                              # the source and the 5 bytes in front of it: as far back as the dictionary goes
        L = Lay(rng, 2500)
        L.put(2000 - 5, d[:29] + bytes([d[29] ^ 0x5A]))
        L.fill(1300, 200, 500)
        return L.bytes(), dict(p=2000)
    yield Case("dict/back_stops_at_the_seam/dictionary_side", dict_first_byte, frs, attempts=1, dictionary=hidden_dict, decides=dict_decides)

    def sides(longest_in_dict):
        def recipe(rng, d):
            L = Lay(rng, 3000)
            body = d[400:440] + L.rnd(8)
            L.cand(300, body, 12 if longest_in_dict else 46)
            L.target(2000, body)
            return L.bytes(), dict(p=2000)
        return recipe
    yield Case("dict/longest_in_the_dictionary", sides(True), frs, dictionary=_dict_of(1024), decides=dict_decides)
    yield Case("dict/longest_in_the_input", sides(False), frs, dictionary=_dict_of(1024), decides=dict_decides)

    def costs(rng):
        d = bytearray(unique_stream(rng, 1024))
        body = bytes(rng.integers(0, 256, 48, dtype=np.uint8))
        d[100:131] = body[:30] + bytes([body[30] ^ 0x5A])     # the third on the chain: 30 bytes
        d[1018:1024] = body[:6]                               # the second: 6 bytes to the seam, which cannot beat the first's 10
        return bytes(d)

    def costs_input(rng, d):
        L = Lay(rng, 3000)
        body = d[100:130] + L.rnd(18)
        L.cand(300, body, 10)
        L.target(2000, body)
        return L.bytes(), dict(p=2000, k=3)
    for A in (2, 3):
        yield Case("dict/a_passed_over_candidate_costs_an_attempt/A%d" % A, costs_input, frs, attempts=A, dictionary=costs,
                   decides=costs_decide)

    def sizes(rng, d):                                        # records shorter and longer than the dictionary
        return bytes(d[200:260]) + bytes(unique_stream(rng, 20)) + bytes(d[10:40]), {}
    yield Case("dict/record_shorter_than_the_dictionary", sizes, frs, dictionary=_dict_of(1024), decides=dict_decides)

    def second_chunk(rng, d):                                 # copies of the dictionary and of the first chunk, in the second
        L = Lay(rng, CHUNK + 3000)
        L.put(200, d[-300:-100]); L.fill(6000, 5000)
        L.put(CHUNK + 500, d[-200:]); L.put(CHUNK + 1000, L.get(100, 300)); L.put(CHUNK + 1500, L.get(CHUNK - 100, 90))
        return L.bytes(), {}
    yield Case("dict/second_chunk_does_not_see_it", second_chunk, ("i256", "l64"), dictionary=_dict_of(1024), decides=dict_decides)


def cases() -> list:
    out = []
    for gen in (_pick_cases, _attempts_cases, _lazy_cases, _back_cases, _long_cases, _seam_cases, _end_cases, _text_cases, _raw_cases,
                _dict_cases):
        out += list(gen())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CORPUS = None


def corpus() -> list:
    global _CORPUS
    if _CORPUS is None: _CORPUS = cases()
    return _CORPUS


FAMILIES = ("pick", "attempts", "lazy", "back", "long", "seam", "end", "text", "raw", "dict")


def select(fam: str, fr: str) -> list:
    return [c for c in corpus() if c.fam == fam and fr in c.framings]
