"""Pass E1's tile merge (csrc/encode.cuh: e1_merge): a numpy / Python model and the tiles the tests run through it and through the kernel.

A tile (64 KiB, positions ts .. te, its block ends at bend) is searched in slices of 128 bytes, each parsed as if nothing in front of it
reached into it.  What the search leaves per slice: s_end (the end of its last match, 0: none), s_n (records found) and a list of
records {literals since the record before or the slice's start, match length, offset}, 32 slots per slice - a helping of several
slices writes one list, into its first slice's slots and on into the next ones'.  The merge is the sequential walk over the slices in
order: the running cover (the maximum of the s_end in front, at least ts), E1Walk::step's keep / shorten / drop, pack_rec with the
literal runs counted from the kept match in front, and the ChunkInfo fields.  `model` is that walk; `reserve` says what the pool's bump
pointer is advanced by - the records kept (the form before round 7) or the records found (E1_V9: an upper bound, known before the walk).

The cases are the smallest shapes at which a merge can go wrong (one tile each); see `cases()`.
"""
import numpy as np

E1_TILE, E1_SLICE, E1_NSLICE, E1_REC_PER_SLICE = 65536, 128, 512, 32
MINMATCH, MFLIMIT, LASTLIT = 4, 12, 5
N_CHUNKS, CHUNK = 3, 1                    # the probe's workspace: three chunks, the tile is the middle one


def rec_pool_at(n_chunks):
    return 8 + ((n_chunks + 1 + 15) // 16) * 8


def len_ext_bytes(v):
    return (v - 15) // 255 + 1 if v >= 15 else 0


def seq_size(lit, mlen):
    return 1 + len_ext_bytes(lit) + lit + 2 + len_ext_bytes(mlen - MINMATCH)


def pack_rec(lit, mlen, off):
    return lit | (mlen << 24) | (off << 48)


class Tile:
    """One tile as the search leaves it.  pool: records the pool holds; bump0: what its bump pointer stands at when the merge begins."""

    def __init__(self, name, ts=3 * E1_TILE, tlen=E1_TILE, bend=None, pool=1 << 15, bump0=0):
        self.name, self.ts, self.te = name, ts, ts + tlen
        self.bend = (self.te + (E1_TILE if tlen == E1_TILE else 0)) if bend is None else bend      # (a short tile is its block's last)
        assert 0 < tlen <= E1_TILE and self.bend >= self.te
        self.nslice = (tlen + E1_SLICE - 1) // E1_SLICE
        self.pool, self.bump0 = pool, bump0
        self.s_end = np.zeros(E1_NSLICE, dtype=np.uint32)
        self.s_n = np.zeros(E1_NSLICE, dtype=np.uint8)
        self.lists = np.zeros(E1_NSLICE * E1_REC_PER_SLICE, dtype=np.uint64)

    @property
    def end_lim(self):                     # where a match may end
        return min(self.te, self.bend - LASTLIT)

    def put(self, s, recs):
        """slice s's list: recs = [(start, mlen, offset)] in absolute positions, ascending, not overlapping each other"""
        pos = self.ts + s * E1_SLICE
        assert s < self.nslice and len(recs) <= 255 and s * E1_REC_PER_SLICE + len(recs) <= self.lists.size
        for i, (st, ml, off) in enumerate(recs):
            assert st >= pos and ml >= MINMATCH and st + ml <= self.end_lim and st + MFLIMIT <= self.bend and 1 <= off <= 65535, (self.name, s, i, st, ml, off)
            self.lists[s * E1_REC_PER_SLICE + i] = pack_rec(st - pos, ml, off)
            pos = st + ml
        self.s_n[s] = len(recs)
        self.s_end[s] = pos if recs else 0
        return self

    def stale(self, rng):
        """what an earlier, longer tile left behind nslice: match ends, counts and records that the merge must not look at"""
        n = self.nslice
        self.s_end[n:] = rng.integers(self.ts, self.ts + E1_TILE, E1_NSLICE - n, dtype=np.uint32)
        self.s_n[n:] = rng.integers(1, E1_REC_PER_SLICE + 1, E1_NSLICE - n, dtype=np.uint8)
        self.lists[n * E1_REC_PER_SLICE:] = [pack_rec(3, 9, 77)] * ((E1_NSLICE - n) * E1_REC_PER_SLICE)
        return self


def model(t, reserve):
    """-> dict(recs: packed records kept, nrec, first_lit, tail_lit, body_size, mode, room, bump: the bump pointer afterwards, noroom, found)"""
    assert reserve in ("kept", "found")
    cov, kept = t.ts, []
    for s in range(t.nslice):
        pos = t.ts + s * E1_SLICE
        for r in range(int(t.s_n[s])):
            x = int(t.lists[s * E1_REC_PER_SLICE + r])
            lit, mlen, off = x & 0xFFFFFF, (x >> 24) & 0xFFFFFF, x >> 48
            start = pos + lit
            end = pos = start + mlen
            if end <= cov:
                continue
            if start < cov:                  # straddles: what is left of it, if that is still a match
                if end - cov < MINMATCH or cov + MFLIMIT > t.bend:
                    continue
                start, mlen = cov, end - cov
            kept.append((start, mlen, off))
        cov = max(cov, int(t.s_end[s]))
    recs, le, body = [], t.ts, 0
    for st, ml, off in kept:
        assert st >= le, (t.name, st, le)
        recs.append(pack_rec(st - le, ml, off))
        body += seq_size(st - le, ml)
        le = st + ml
    found = int(t.s_n[:t.nslice].astype(np.int64).sum())
    want = len(kept) if reserve == "kept" else found
    base = t.bump0 if want else 0          # (nothing to reserve: the bump pointer is not asked)
    room = base + want <= t.pool
    out = dict(recs=np.array(recs, dtype=np.uint64), nrec=len(kept), first_lit=(kept[0][0] - t.ts) if kept else 0, tail_lit=t.te - le, body_size=body,
               mode=2 if len(kept) * 64 > t.te - t.ts else 1, room=room, bump=t.bump0 + want, noroom=0 if room else 1, found=found, base=base)
    if not room:                             # the tile goes out as literals
        out.update(recs=np.zeros(0, dtype=np.uint64), nrec=0, first_lit=0, tail_lit=t.te - t.ts, body_size=0)
    return out


def unpack(recs, ts):
    """packed kept records -> [(start, mlen, off)]"""
    out, pos = [], ts
    for x in (int(v) for v in recs):
        st = pos + (x & 0xFFFFFF)
        ml = (x >> 24) & 0xFFFFFF
        out.append((st, ml, x >> 48))
        pos = st + ml
    return out


# ------------------------------------------------------------------------------------------ the cases
def _bench_shape(name, **kw):
    """rows of 1 KiB, 512 random bytes and their copy: a helping of eight slices finds one record, in its first slice's list"""
    t = Tile(name, **kw)
    for s in range(0, t.nslice, 8):
        cs = t.ts + s * E1_SLICE
        if cs + 1024 <= t.end_lim:
            t.put(s, [(cs + 515, 509, 512)])
    return t


def _short_matches(t, s, n, gap=0, mlen=MINMATCH, off=9):
    cs = t.ts + s * E1_SLICE
    return t.put(s, [(cs + i * (mlen + gap) + gap, mlen, off) for i in range(n)])


def _mixed_lists(name, counts):
    """slice s holds counts[s % len(counts)] records of four bytes (32 of them fill a slice): nothing overlaps, everything is kept"""
    t = Tile(name)
    for s in range(t.nslice):
        n = counts[s % len(counts)]
        if n:
            _short_matches(t, s, n)
    return t


def _cover(name, k, extra):
    """slice 40's second record reaches over the next k slices and `extra` bytes into the one after: the lists of the slices under it are
    dropped whole, the list of the one it ends in loses what lies under it, and the record that straddles its end is shortened"""
    t = Tile(name)
    s0 = 40
    cs = t.ts + s0 * E1_SLICE
    end = cs + (k + 1) * E1_SLICE + extra
    _short_matches(t, s0 - 1, 2, gap=3)
    t.put(s0, [(cs + 10, 20, 300), (cs + 60, end - (cs + 60), 4000)])
    for s in range(s0 + 1, min(s0 + k + 4, t.nslice)):
        c2 = t.ts + s * E1_SLICE
        t.put(s, [(c2 + 5, 30, 11), (c2 + 50, 40, 12), (c2 + 100, 20, 13)] if s % 3 else [(c2 + 2, 100, 14)])
    return t


def _straddle(name, left, bend_gap=None):
    """slice 8's match ends `cut` bytes into slice 9's first record, which has `left` bytes behind that; bend_gap: the block ends that
    many bytes behind the cover (MFLIMIT decides)"""
    if bend_gap is None:
        t = Tile(name)
    else:
        tlen = 10 * E1_SLICE
        t = Tile(name, tlen=tlen, bend=3 * E1_TILE + tlen)
    c8, c9 = t.ts + 8 * E1_SLICE, t.ts + 9 * E1_SLICE
    cov = c9 + 20 if bend_gap is None else t.bend - bend_gap
    t.put(8, [(c8 + 30, cov - (c8 + 30), 100)])
    t.put(9, [(c9 + 2, cov + left - (c9 + 2), 200)] + ([(cov + left + 6, 8, 201)] if bend_gap is None else []))
    return t


def _random_tile(rng, i):
    tlen = E1_TILE if rng.random() < 0.7 else int(rng.integers(1, E1_TILE + 1))
    last = rng.random() < 0.3
    t = Tile("random%03d" % i, tlen=tlen, bend=3 * E1_TILE + tlen + (0 if last else int(rng.integers(0, 1 << 20))), bump0=int(rng.integers(0, 5000)))
    kind = rng.integers(0, 3)                # 0: long helpings (sparse), 1: single slices (dense), 2: both
    p_long = (0.02, 0.002, 0.01)[kind]
    p8 = float(rng.choice([0.01, 0.12]))                        # (... or more than a slice's 32 slots: the list runs on into the next slice's)
    cap8 = 2 if kind == 0 and rng.random() < 0.4 else 60      # (long helpings that found at most two records each: the merge's straight-line form)
    s = 0
    while s < t.nslice:
        grab = 8 if kind == 0 or (kind == 2 and rng.random() < 0.5 and s % 8 == 0) else 1
        cs = t.ts + s * E1_SLICE
        ce = min(cs + grab * E1_SLICE, t.te)
        recs, pos = [], cs
        density = rng.choice([0.0, 0.3, 1.0, 1.0]) if grab == 1 else rng.choice([0.0, 1.0, 1.0])
        while density and len(recs) < (E1_REC_PER_SLICE if grab == 1 else cap8):
            lit = int(rng.geometric(0.15 if grab == 1 else p8 if cap8 > 2 else 0.004)) - 1 if rng.random() < density else 10 ** 6
            st = pos + lit
            if st >= ce or st + MINMATCH > t.end_lim or st + MFLIMIT > t.bend:
                break
            ml = int(rng.integers(MINMATCH, 24)) if rng.random() > p_long else int(rng.integers(24, 40000))
            ml = min(ml, t.end_lim - st)
            recs.append((st, ml, int(rng.integers(1, 65536))))
            pos = st + ml
            if pos >= ce:
                break
        t.put(s, recs)
        s += grab
    if t.nslice < E1_NSLICE:
        t.stale(rng)
    return t


def cases():
    """[Tile].  Every case is one tile; all but the two `pool_*` ones have a pool that both reservation rules find roomy."""
    rng = np.random.default_rng(20240707)
    out = [Tile("empty"), Tile("empty_short", tlen=1000).stale(rng), _bench_shape("bench"), _bench_shape("bench_bump", bump0=4321)]
    # lists of 0, 1, 2, 3, 4 and 32 records: at most two everywhere (straight-line code), exactly three somewhere (the loop), and all mixed
    out += [_mixed_lists("lists_le2", [0, 1, 2, 2, 1, 0, 2]), _mixed_lists("lists_3", [0, 1, 2] * 40 + [3]), _mixed_lists("lists_mixed", [0, 1, 2, 3, 4, 32, 0, 32, 1])]
    t = Tile("lists_one_long")               # one list of 32 in a tile of short ones, in the last lane's last slice
    for s in range(0, t.nslice - 1, 5):
        _short_matches(t, s, 1 + s % 2, gap=2)
    out.append(_short_matches(t, t.nslice - 1, 32))
    # a record that covers the next 1, 7, 8, 9, 64 and 300 slices: lanes in the middle keep nothing, the cover crosses lane boundaries
    out += [_cover("cover_%d" % k, k, extra) for k, extra in ((1, 7), (7, 60), (8, 1), (9, 127), (64, 33), (300, 51))] + [_cover("cover_1_to_the_byte", 1, 0)]
    # a straddling record shortened to exactly MINMATCH (kept), to MINMATCH - 1 (dropped), and one dropped because the block ends
    out += [_straddle("straddle_keep4", MINMATCH), _straddle("straddle_drop3", MINMATCH - 1), _straddle("straddle_keep5", 5, bend_gap=MFLIMIT),
            _straddle("straddle_mflimit", 5, bend_gap=10)]
    # short tiles with stale words behind them
    for ns in (1, 7, 8, 9, 511):
        tlen = ns * E1_SLICE - 37
        t = Tile("nslice_%d" % ns, tlen=tlen, bend=3 * E1_TILE + tlen + (0 if ns != 9 else 5000))
        for s in range(t.nslice):
            cs = t.ts + s * E1_SLICE
            if cs + 40 <= t.end_lim:
                t.put(s, [(cs + 3, min(30, t.end_lim - cs - 3), 5)] if s % 2 == 0 else [(cs + 1, 6, 6), (cs + 20, 5, 7)])
        out.append(t.stale(rng))
    # the cover is ts where nothing has matched yet: the first record sits in the sixth lane's slices, and one in the last slice only
    t = Tile("first_in_lane5")
    out.append(_short_matches(t, 43, 2, gap=5))
    out.append(_short_matches(Tile("last_slice_only"), E1_NSLICE - 1, 1, gap=60))
    # the pool: exactly enough room and one record short (nothing is dropped in these tiles: found == kept, both rules agree)
    for name, short in (("pool_exact", 0), ("pool_short1", 1)):
        t = _bench_shape(name, bump0=1000)
        t.pool = t.bump0 + int(t.s_n.sum()) - short
        out.append(t)
    out += [_random_tile(rng, i) for i in range(200)]
    names = [t.name for t in out]
    assert len(set(names)) == len(names)
    return out
