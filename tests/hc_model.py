"""A sequential model of the hash-chain encoder of levels 3-12 (test helper, not a test module; numpy only, nothing of the library).

Written from csrc/encode_hc.cuh's header, DESIGN.md section 4 ("High-compression levels") and LZ4HC's definition: what the records
of a 64 KiB chunk are, as a function of the input, its history, the framing, the level and the dictionary.  tests/test_hc_model_cpu.py
holds the model to a hash-free definition of the search and to the block format; tests/test_gpu_hc_model.py holds the kernels to the
model, byte for byte.

Per chunk of a block (64 KiB, the last one shorter):
  window     the chunk and the `back` = min(64 KiB, chunk start - low) bytes in front of it; low is the block's start, the input's
             when blocks are linked.  Positions count from the window's first byte.
  limits     last_start = min(chunk end - 4, block end - 12): the last position a match may start at;  end_lim = min(chunk end,
             block end - 5): where a match ends at the latest.  A block under 13 bytes, a chunk under 4, or last_start in front of
             the chunk: the chunk is literals.
  chain      every window position <= last_start is a candidate for the later ones with the same 13-bit hash of its 4 bytes
  search     every chunk position p <= last_start: the earlier positions with p's hash, nearest first, none further back than
             65535, at most `attempts` of them.  One whose 4 bytes are p's matches for the common prefix, at most min(258,
             end_lim - p); a strictly longer one replaces the best; the walk ends when the best is at that cap.  With the best go
             the bytes it also matches backwards: at most 255, not below the chunk's start nor the window's first byte.
  parse      from the pending anchor to the first position with a match; while that is under 258: on to p+1 if p+1's is longer,
             else (lazy 2) to p+2 if p+2's is longer by more than one.  The match is taken, pulled back into the pending literals
             as far as it extends, and one of 258 runs on to the first difference or end_lim.
  dictionary the last min(64 KiB, len) bytes of the dictionary lie in front of a scope's first chunk only (a scope: an independent
             block, a linked frame).  The seam cuts every match: a candidate in the dictionary ends at the dictionary's last byte
             and extends backwards within it; a candidate in the input does not extend backwards below the seam; positions whose 4
             bytes straddle the seam are no candidates.  A dictionary candidate that cannot beat the best still costs an attempt.
             A dictionary under 4 bytes is ignored.

None of this depends on how the kernel schedules its work.  Window.schedule restates that schedule as well (batches of 960
positions, the parse's 64-lane window), only to say in which lane of which window the parse stood when it took a match: the cases
that are placed by lane are checked with it.

Attempts are counted over positions with the same hash within reach.  (The kernel's chain has false links: an empty head entry
links a chain's end to window position 0 or 65536, and a predecessor 65536 or more back leaves an aliased 16-bit distance.  Both
can only follow the last true candidate within reach, and from there on the walk sees only positions of other hashes, whose 4 bytes
differ: they spend attempts that no true candidate is left to use.)
"""
from __future__ import annotations

import bisect

import numpy as np

CHUNK = 1 << 16
REACH = 65535
CAP = 258                                                    # the longest match a search records
BACK_CAP = 255                                               # the most bytes a search records backwards
MINMATCH, MFLIMIT, LASTLIT = 4, 12, 5
HASH_LOG = 13
ATTEMPTS = (32, 48, 64, 256, 384, 512, 1024, 2048, 4096, 8192)      # levels 3..12 (DESIGN.md's table)
UNLIMITED = 1 << 30


def level_params(level: int) -> tuple:
    """(attempts, lazy look-ahead) of a compression level 3..12; above 12 is 12."""
    level = min(max(level, 3), 12)
    return ATTEMPTS[level - 3], 2 if level >= 6 else 1


def ext(v: int) -> int:
    """Length bytes behind a token's nibble."""
    return (v - 15) // 255 + 1 if v >= 15 else 0


def seq_size(lit: int, mlen: int) -> int:
    return 1 + ext(lit) + lit + 2 + ext(mlen - 4)


def _w32(w: np.ndarray) -> np.ndarray:
    a = np.zeros(len(w) + 3, np.uint32)
    a[:len(w)] = w
    return a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)


def _w64(w: np.ndarray) -> np.ndarray:
    """The 8 bytes at every position as a little-endian word (zeros behind the end)."""
    n = len(w)
    m = n // 8 + 2
    pad = np.zeros(8 * m + 8, np.uint8)
    pad[:n] = w
    raw = pad.tobytes()
    out = np.empty(8 * m, np.uint64)
    for k in range(8):
        out[k::8] = np.frombuffer(raw[k:k + 8 * m], "<u8")
    return out


def _prefix(w64, a, b, cap, start):
    """Per pair: the common prefix of what begins at a and at b, given that the first `start` bytes are equal; at most cap."""
    ln = np.minimum(np.full(len(a), start, np.int64), cap)
    live = np.flatnonzero(ln < cap)
    while len(live):
        x = w64[a[live] + ln[live]] ^ w64[b[live] + ln[live]]
        nz = x != 0
        add = np.full(len(live), 8, np.int64)
        if nz.any():
            add[nz] = (np.ascontiguousarray(x[nz]).astype("<u8").view(np.uint8).reshape(-1, 8) != 0).argmax(axis=1)
        ln[live] += add
        live = live[~nz & (ln[live] < cap[live])]
    return np.minimum(ln, cap)


class Window:
    """One chunk's window and limits.  w: the window's bytes (a dictionary's tail first, if it has one); seam: the dictionary's
    bytes in it; cs: the chunk's first position; searchable: whether a match may start in the chunk at all."""

    def __init__(self, w: np.ndarray, seam: int, cs: int, clen: int, to_block_end: int, blen: int):
        self.w, self.seam, self.cs, self.ce = w, seam, cs, cs + clen
        bend = self.ce + to_block_end
        self.searchable = blen >= MFLIMIT + 1 and clen >= MINMATCH
        self.last_start = self.end_lim = -1
        if self.searchable:
            self.last_start = min(self.ce - MINMATCH, bend - MFLIMIT)
            self.end_lim = min(self.ce, bend - LASTLIT)
            self.searchable = self.last_start >= cs
        self._found = {}

    def search(self, attempts_list, back: bool = True) -> dict:
        """attempts -> (L, O, B): per window position the best match's length (0: none), offset and backward extension."""
        todo = sorted(set(a for a in attempts_list if (a, back) not in self._found))
        if todo:
            for a, r in self._search(todo, back).items(): self._found[a, back] = r
        return {a: self._found[a, back] for a in attempts_list}

    def _search(self, todo, back):
        w, seam, cs, last_start, end_lim = self.w, self.seam, self.cs, self.last_start, self.end_lim
        n = len(w)
        out = {}
        if not self.searchable:
            z = np.zeros(n + 3, np.int64)
            return {a: (z, z, z) for a in todo}
        w32, w64 = _w32(w), _w64(w)
        h = ((w32.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_LOG)
        ins = np.arange(0, last_start + 1)
        if seam: ins = ins[(ins < seam - 3) | (ins >= seam)]                  # (their 4 bytes straddle the seam)
        order = ins[np.argsort(h[ins], kind="stable")]
        prev = np.full(n, -1, np.int64)
        same = h[order[1:]] == h[order[:-1]]
        prev[order[1:][same]] = order[:-1][same]
        P = np.arange(cs, last_start + 1)
        maxlen = np.minimum(CAP, end_lim - P)
        best, boff, q = np.zeros(len(P), np.int64), np.zeros(len(P), np.int64), P.copy()
        live = np.arange(len(P))
        step = 0
        for a in todo:
            while step < a and len(live):
                step += 1
                qn = prev[q[live]]
                ok = (qn >= 0) & (P[live] - qn <= REACH)
                live, qn = live[ok], qn[ok]
                q[live] = qn
                p, cmax, b = P[live], maxlen[live], best[live]
                if seam: cmax = np.where(qn < seam, np.minimum(cmax, seam - qn), cmax)
                c = np.flatnonzero((cmax >= MINMATCH) & (cmax > b) & (w32[qn] == w32[p]))
                if len(c): c = c[w[qn[c] + b[c]] == w[p[c] + b[c]]]           # (a longer match has the byte at `best` too)
                if len(c):
                    ln = _prefix(w64, p[c], qn[c], cmax[c], MINMATCH)
                    better = ln > b[c]
                    at = live[c[better]]
                    best[at], boff[at] = ln[better], p[c[better]] - qn[c[better]]
                live = live[best[live] < maxlen[live]]
            bk = np.zeros(len(P), np.int64)
            m = np.flatnonzero(best >= MINMATCH)
            if back and len(m):
                p, qb = P[m], P[m] - boff[m]
                room = np.minimum(np.minimum(p - cs, np.where(qb >= seam, qb - seam, qb)), BACK_CAP)
                k = np.zeros(len(m), np.int64)
                lv = np.flatnonzero(room > 0)
                while len(lv):
                    lv = lv[w[p[lv] - 1 - k[lv]] == w[qb[lv] - 1 - k[lv]]]
                    k[lv] += 1
                    lv = lv[k[lv] < room[lv]]
                bk[m] = k
            L, O, B = np.zeros(n + 3, np.int64), np.zeros(n + 3, np.int64), np.zeros(n + 3, np.int64)
            L[cs:last_start + 1], O[cs:last_start + 1], B[cs:last_start + 1] = best, boff, bk
            out[a] = (L, O, B)
        return out

    def parse(self, attempts: int, lazy: int, back: bool = True):
        """-> (records [(literals, match length, offset)], the chunk's final literals, events [(position taken, position the parse
        first stood on, window position of the match's source)])."""
        cs, ce, w, seam, end_lim = self.cs, self.ce, self.w, self.seam, self.end_lim
        if not self.searchable: return [], ce - cs, []
        L, O, B = (x.tolist() for x in self.search([attempts], back)[attempts])
        has = [i for i, v in enumerate(L) if v]
        recs, events = [], []
        anchor = p = cs
        while True:
            i = bisect.bisect_left(has, p)
            if i == len(has): break
            p = first = has[i]
            while L[p] < CAP:
                if L[p + 1] > L[p]: p += 1
                elif lazy >= 2 and L[p + 2] > L[p] + 1: p += 2
                else: break
            mlen, off = L[p], O[p]
            bk = min(B[p], p - anchor)
            if mlen >= CAP:
                lim = end_lim
                if p - off < seam: lim = min(lim, p + seam - (p - off))
                a = p + mlen
                if a < lim:
                    ne = np.flatnonzero(w[a:lim] != w[a - off:lim - off])
                    mlen += int(ne[0]) if len(ne) else lim - a
            recs.append((p - bk - anchor, mlen + bk, off))
            events.append((p, first, p - off))
            anchor = p = p + mlen
        return recs, ce - anchor, events


    def schedule(self, attempts: int, lazy: int, back: bool = True) -> dict:
        """Where each taken match stood in the parse's 64-lane window, as the kernel's header schedules the parse: the window is
        walked in batches of 960 positions; in iteration `it` the results of positions below known_end = (it - 1) * 960 are there
        (all of them in the last one), and the parse goes on while p + 2 < known_end.  It loads 64 results from p on and decides the
        positions whose look-ahead is loaded and known, p .. min(p + 62, known_end - 2); a lazy move that lands beyond them is
        decided again after the next load.  -> {position taken: dict(w0: the window's first position, lane: the taken position's
        lane, first: the lane the parse first stood on in the window the event began in, full: that window was 62 positions wide,
        reloads: loads between the first stand and the taking)}.  The positions taken are parse()'s: the schedule decides nothing."""
        out = {}
        if not self.searchable: return out
        recs, _, events = self.parse(attempts, lazy, back)
        after, anchor = {}, self.cs                          # position taken -> where the parse goes on
        for (lit, ml, _), (p, _, _) in zip(recs, events):
            anchor += lit + ml
            after[p] = anchor
        L = self.search([attempts], back)[attempts][0].tolist() + [0] * 70
        T, last_start = 960, self.last_start
        nbatch = (last_start + 1 + T - 1) // T
        p = self.cs
        began = None                                         # (w0, lane, full) of the window the pending event began in, loads since
        for it in range(self.seam // T, nbatch + 2):
            fin = it == nbatch + 1
            known_end = (it - 1) * T if it >= 1 else 0
            while p <= last_start and (fin or p + 2 < known_end):
                w0 = p
                wend = w0 + 62 if fin else min(w0 + 62, known_end - 2)
                while p < wend:
                    nxt = next((x for x in range(p, wend) if L[x]), None)
                    if nxt is None:
                        p = wend
                        break
                    p = nxt
                    if began is None: began = [w0, p - w0, wend == w0 + 62, 0]
                    moved = False
                    while L[p] < CAP:
                        if L[p + 1] > L[p]: p += 1
                        elif lazy >= 2 and L[p + 2] > L[p] + 1: p += 2
                        else: break
                        moved = True
                        if p >= wend: break
                    if moved and p >= wend:
                        began[3] += 1
                        break
                    assert p in after, p
                    out[p] = dict(w0=w0, lane=p - w0, first=began[1], first_w0=began[0], full=began[2], reloads=began[3])
                    began = None
                    p = after[p]
        assert sorted(out) == sorted(after), "the schedule takes what the parse takes"
        return out


class Model:
    """The encoder's records for `data` in blocks of bs bytes, linked or not, with a dictionary or without."""

    def __init__(self, data: bytes, bs: int, linked: bool, dictionary: bytes = b""):
        self.data, self.bs, self.linked = bytes(data), bs, linked
        self.dict = bytes(dictionary)[-CHUNK:] if len(dictionary) >= MINMATCH else b""
        d = np.frombuffer(self.data, np.uint8)
        dd = np.frombuffer(self.dict, np.uint8)
        self.windows = []                                    # (block start, chunk start, Window)
        n = len(d)
        for b0 in range(0, n, bs):
            blen = min(bs, n - b0)
            low = 0 if linked else b0
            for c0 in range(b0, b0 + blen, CHUNK):
                clen = min(CHUNK, b0 + blen - c0)
                if c0 == low and len(dd): w, seam, back = np.concatenate([dd, d[c0:c0 + clen]]), len(dd), len(dd)
                else:
                    back = min(CHUNK, c0 - low)
                    w, seam = d[c0 - back:c0 + clen], 0
                self.windows.append((b0, c0, Window(w, seam, back, clen, b0 + blen - (c0 + clen), blen)))

    def parse(self, level: int | None = None, attempts: int | None = None, lazy: int | None = None, back: bool = True) -> "Parse":
        a, z = level_params(level if level is not None else 12)
        return Parse(self, attempts if attempts is not None else a, lazy if lazy is not None else z, back)


class Parse:
    """chunks: per chunk (block start, chunk start, records, final literals, events - positions in the window);
    blocks: per block dict(start, blen, seqs [(literals, match length, offset)], final, size, stored);
    rows: (position in the input, length, offset, literals in front), neighbours merged as lz4_writer_rules.matches merges them."""

    def __init__(self, m: Model, attempts: int, lazy: int, back: bool):
        self.model, self.attempts, self.lazy = m, attempts, lazy
        self.chunks = [(b0, c0) + win.parse(attempts, lazy, back) + (win,) for b0, c0, win in m.windows]
        self.blocks = []
        for b0 in range(0, len(m.data), m.bs):
            blen = min(m.bs, len(m.data) - b0)
            seqs, carry = [], 0
            for cb, c0, recs, tail, _, _ in self.chunks:
                if cb != b0: continue
                for k, (lit, ml, off) in enumerate(recs):
                    seqs.append((lit + carry if k == 0 else lit, ml, off))
                if recs: carry = tail
                else: carry += tail
            size = sum(seq_size(l, ml) for l, ml, _ in seqs) + 1 + ext(carry) + carry
            self.blocks.append(dict(start=b0, blen=blen, seqs=seqs, final=carry, size=size, stored=size >= blen))
        rows = []
        for B in self.blocks:
            if B["stored"]: continue
            at = B["start"]
            for lit, ml, off in B["seqs"]:
                pos = at + lit
                if lit == 0 and rows and rows[-1][2] == off and rows[-1][0] + rows[-1][1] == pos and pos > B["start"]: rows[-1][1] += ml
                else: rows.append([pos, ml, off, lit])
                at = pos + ml
        self.rows = np.array(rows, dtype=np.int64).reshape(-1, 4)

    @property
    def stored(self) -> list:
        return [k for k, B in enumerate(self.blocks) if B["stored"]]

    def payload(self, k: int) -> bytes:
        """Block k as the block format writes its sequences (or its bytes as they are, when it is stored)."""
        B, data = self.blocks[k], self.model.data
        if B["stored"]: return data[B["start"]:B["start"] + B["blen"]]
        out, at = bytearray(), B["start"]

        def put(lit, ml):
            tok = (min(lit, 15) << 4) | (min(ml - 4, 15) if ml else 0)
            out.append(tok)
            if lit >= 15:
                v = lit - 15
                out.extend(b"\xff" * (v // 255)); out.append(v % 255)
            out.extend(data[at:at + lit])

        for lit, ml, off in B["seqs"]:
            put(lit, ml)
            out.extend((off & 255, off >> 8))
            if ml - 4 >= 15:
                v = ml - 19
                out.extend(b"\xff" * (v // 255)); out.append(v % 255)
            at += lit + ml
        put(B["final"], 0)
        assert len(out) == B["size"] and at + B["final"] == B["start"] + B["blen"]
        return bytes(out)

    def frame_size(self, header: int = 7, bck: bool = False, cck: bool = False) -> int:
        return header + sum(4 + (B["blen"] if B["stored"] else B["size"]) + 4 * int(bck) for B in self.blocks) + 4 + 4 * int(cck)

    def frame(self, header: bytes) -> bytes:
        """The whole frame behind `header` (no checksums)."""
        out = bytearray(header)
        for k, B in enumerate(self.blocks):
            pay = self.payload(k)
            out += (len(pay) | (0x80000000 if B["stored"] else 0)).to_bytes(4, "little") + pay
        return bytes(out + bytes(4))


def exhaustive(win: Window):
    """The search without hash or chain: per chunk position the longest match among ALL earlier window positions within reach
    whose 4 bytes are equal, the nearest among equals, under the same caps.  -> (L, O) as Window.search gives them."""
    w, seam, cs, last_start, end_lim = win.w, win.seam, win.cs, win.last_start, win.end_lim
    n = len(w)
    L, O = np.zeros(n + 3, np.int64), np.zeros(n + 3, np.int64)
    if not win.searchable: return L, O
    P = np.arange(cs, last_start + 1)
    maxlen = np.minimum(CAP, end_lim - P)
    best, boff = np.zeros(len(P), np.int64), np.zeros(len(P), np.int64)
    for d in range(1, min(last_start, REACH) + 1):
        p = P[P >= d]
        if not len(p): break
        q = p - d
        eq = w[d:] == w[:-d]                                  # eq[i]: w[i + d] == w[i]
        stop = np.append(np.flatnonzero(~eq), n - d)
        run = stop[np.searchsorted(stop, q)] - q              # equal bytes from q on
        cmax = maxlen[p - cs]
        if seam:
            cmax = np.where(q < seam, np.minimum(cmax, seam - q), cmax)
            run = np.where((q >= seam - 3) & (q < seam), 0, run)
        ln = np.minimum(run, cmax)
        ln = np.where(ln >= MINMATCH, ln, 0)
        better = ln > best[p - cs]
        best[p[better] - cs], boff[p[better] - cs] = ln[better], d
    L[cs:last_start + 1], O[cs:last_start + 1] = best, boff
    return L, O
