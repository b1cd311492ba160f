"""The walk cases (tests/walk_cases.py) held to the oracle, to a plain walk, and to the walks' documented rules.  No GPU.

Per case: the oracle's verdict on the buffer equals the plain Python walk's (walk_cases.model_record), which is the record the
GPU test expects; the documented candidate rule (frame_dev.cuh: a position whose word passes the hop rule of frame_format.hpp
for K hops, or up to an EndMark), restated here, finds nothing in a must_deliver case but the true size words, the planted
decoys, a second chain's words, and stray positions that nobody points at; and the documented filter and link rules, restated,
give the outcome the case's name is listed under.  So a must_deliver expectation does not rest on luck.  The seeded cases are
checked at a few blocks (walk_cases.seeded_small); the GPU test makes them at full size from the same operations."""
import ctypes

import numpy as np
import pytest

import frame_edges as fe
import walk_cases as wc


def small(name):
    return wc.seeded_small(name) if name.startswith("seed/") else wc.case(name)


# ---- the documented rules, restated ---------------------------------------------------------------------------------------------
def step(a, cap, bs, bck, pos):
    """The hop rule: the word at pos -> (position of the next word, the word is an EndMark), or None where no walk goes on."""
    if pos > cap or cap - pos < 4: return None
    w = wc.u32(a[pos:pos + 4])
    n = w & 0x7FFFFFFF
    adv = 0 if w == 0 else n + 4 * bck
    if n > bs or cap - pos - 4 < adv: return None
    nxt = pos + 4 + adv
    if w != 0 and cap - nxt < 4: return None
    return nxt, w == 0


def candidates(a, c, hops):
    """Every position from the header on that the candidate rule takes, in order."""
    cap, bs, bck = c.cap, c.bs, c.bck
    top = a[3:cap]
    at = np.flatnonzero((top == 0) | (top == 0x80))
    v = (a[at].astype(np.uint32) | (a[at + 1].astype(np.uint32) << 8) | (a[at + 2].astype(np.uint32) << 16) | (a[at + 3].astype(np.uint32) << 24))
    hi_mask = ~((bs << 1) - 1) & 0x7FFFFFFF
    at = at[((v & hi_mask) == 0) & (v != 0) & (at >= c.hsize)]
    out = []
    for p in at.tolist():
        q, good = p, True
        for h in range(hops):
            r = step(a, cap, bs, bck, q)
            if r is None or (h == 0 and r[1]): good = False; break
            if r[1]: break
            q = r[0]
        if good: out.append(p)
    return out


def list_verdict(a, c, lst, exact=False):
    """k_walk_link / k_walk_verdict: the number of blocks the list delivers, or None where it is declined."""
    cap, bs, bck, total = c.cap, c.bs, c.bck, len(lst)
    table_cap = min(c.room // bs + 2, cap // 5 + 2)
    if total == 0 or lst[0] != c.hsize:
        if cap - c.hsize < 4 or wc.u32(a[c.hsize:c.hsize + 4]) != 0 or (exact and total): return None
        n, pos = 0, c.hsize + 4
    else:
        first_end = first_break = None
        for i, p in enumerate(lst):
            r = step(a, cap, bs, bck, p)
            ok, last = r is not None and not r[1], False
            if ok:
                r2 = step(a, cap, bs, bck, r[0])
                last = r2 is not None and r2[1]
                ok = last or (i + 1 < total and lst[i + 1] == r[0])
            if not ok: first_break = i if first_break is None else first_break
            elif last: first_end = i if first_end is None else first_end
        e = first_end
        if e is None or (first_break is not None and first_break <= e) or e >= table_cap or e * bs >= c.room: return None
        if exact and e + 1 != total: return None
        n = e + 1
        pos = lst[e] + 4 + (wc.u32(a[lst[e]:lst[e] + 4]) & 0x7FFFFFFF) + 4 * bck + 4
    if c.cck and cap - pos < 4: return None
    return n


def parallel_walk(a, c):
    """k_walk_cand .. k_walk_filter on the buffer -> (all candidates, the filtered list, or None after an overflow exit)."""
    C = candidates(a, c, wc.WK_HOPS)
    per_chunk = {}
    for p in C: per_chunk[p // wc.WK_CHUNK] = per_chunk.get(p // wc.WK_CHUNK, 0) + 1
    list_cap = min(c.room // c.bs + 2, c.cap // 5 + 2) + wc.LIST_SLACK
    if any(n > wc.WK_SLOTS for n in per_chunk.values()) or len(C) > list_cap: return C, None
    S, pointed = set(C), set()
    for p in C:
        r = step(a, c.cap, c.bs, c.bck, p)
        if r is not None and not r[1] and r[0] in S: pointed.add(r[0])
    return C, [p for i, p in enumerate(C) if i == 0 or p in pointed]


def head_ok(rec):
    return not rec["host"] and rec["flags"] & 0x100 == 0 and (rec["status"] != wc.ST["frametype"])


@pytest.fixture(scope="module")
def L():
    from lz4_frame_conduit_amd import _ffi
    _ffi.build()
    return _ffi.lib()


# ---- the tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.names())
def test_case_against_oracle_and_rules(name):
    c = small(name)
    a = wc.materialize(c)
    assert a.size == c.cap
    rec = wc.model_record(lambda p, n: a[p:p + n].tobytes(), c.cap, c.room)
    v = fe.verdict(a.tobytes(), c.room)
    assert fe.status_of(v.error) == rec["status"], (name, v.error, rec)
    if v.error is None:
        assert v.consumed == rec["consumed"] and len(v.out) == rec["size"], (name, v.consumed, len(v.out), rec)
        assert rec["flags"] & 0x100 or v.out == wc.content_of(c, a), name
        assert rec["flags"] & 0x100 or (rec["n_blocks"] == len(c.words) == len(c.segs) and c.room >= rec["n_blocks"] * c.bs), name
    # payload-like bytes everywhere but where something was planted
    planted = np.zeros(c.cap, dtype=bool)
    for op in c.ops: planted[op[1]:op[1] + (op[2] if op[0] == "fill" else 4 if op[0] == "xxh" else len(op[2]))] = True
    assert bool(((a[~planted] >= 1) & (a[~planted] <= 0x7F)).all()), name
    assert c.expect == ("must_deliver" if name in wc.MUST_DELIVER else "must_decline" if name in wc.MUST_DECLINE else "free"), name
    sound = v.error is None and not rec["flags"] & 0x100
    assert c.expect != "must_deliver" or sound, name
    if c.kind == "trailer":
        if c.planned == "trailer":
            foot = a[c.cap - 32:].tobytes()
            count, total = wc.u32(foot[20:24]), int.from_bytes(foot[24:32], "little")
            list_at = (c.cap - total + 8 + 15) & ~15
            lst = [int.from_bytes(a[list_at + 8 * i:list_at + 8 * i + 8].tobytes(), "little") for i in range(count)]
            got = list_verdict(a, c, lst, exact=True)
            assert (got == rec["n_blocks"]) if c.expect == "must_deliver" else got is None, (name, got)
            bare = small(c.bare)                                                      # (the same frame without the trailer, payload of its own)
            b = wc.materialize(bare)
            assert wc.model_record(lambda p, n: b[p:p + n].tobytes(), bare.cap, bare.room) == rec, name
        return
    hops = wc.WK_HOPS if c.kind == "parallel" else wc.WK_SEED_HOPS
    C = candidates(a, c, hops)
    known = set(c.words) | set(c.decoys)
    nxt = {p: step(a, c.cap, c.bs, c.bck, p) for p in C}
    pointed = {r[0] for r in nxt.values() if r is not None and not r[1]}
    chained = [p for p in C if p not in known and p in pointed]                       # (a second chain's words behind the frame)
    stray = [p for p in C if p not in known and p not in pointed]
    if c.expect == "must_deliver" or c.decoys:
        assert set(c.decoys) <= set(C) and set(c.words) <= set(C), (name, sorted(set(c.decoys) - set(C)))
        end = rec["consumed"]
        assert all(p >= end for p in chained), (name, chained[:8])
        # a stray: nobody points at it - the filter drops it.  There are none but in front of a second chain, and where zeros lie behind the frame
        assert all(p >= end - 8 - 4 * c.cck for p in stray), (name, stray[:8])
    if c.kind == "parallel" and c.planned == "parallel":
        _, lst = parallel_walk(a, c)
        got = list_verdict(a, c, lst) if lst is not None and head_ok(rec) else None
        print("%s: %d candidates (%d stray), rules say %s" % (name, len(C), len(stray), "declined" if got is None else "delivered, %d blocks" % got))
        if c.expect == "must_deliver": assert got == rec["n_blocks"], (name, got)
        if c.expect == "must_decline": assert got is None, (name, got)


def test_inventory():
    """Every seam the cases are there for is hit by a case, every case is listed under one expectation, and the constants a case is
    built on are the kernels'."""
    cases = [small(n) for n in wc.names()]
    hit = {s for c in cases for s in c.seams}
    assert hit == set(wc.SEAMS), (sorted(set(wc.SEAMS) - hit), sorted(hit - set(wc.SEAMS)))
    assert wc.MUST_DELIVER | wc.MUST_DECLINE | wc.FREE == set(wc.CASES) and not wc.MUST_DELIVER & wc.MUST_DECLINE
    assert not wc.FREE & (wc.MUST_DELIVER | wc.MUST_DECLINE)
    for kind, least in (("par", 55), ("seed", 13), ("trailer", 24)):
        assert len(wc.names(kind)) >= least, kind
    # shifted words: where the name says
    for seam, unit in (("chunk", wc.WK_CHUNK), ("group", wc.WK_GROUP), ("stride", wc.WK_STRIDE)):
        for j in (-3, -2, -1, 0):
            c = wc.case("par/shift/%s%+d" % (seam, j))
            assert (c.words[6] - j) % unit == 0, (seam, j)
    # the constants, against the sources they restate
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "lz4_frame_conduit_amd", "csrc", "frame_dev.cuh")).read()
    for k in ("WK_CHUNK", "WK_SLOTS", "WK_HOPS", "WK_SEEDS", "WK_SEED_HOPS", "WK_SEED_PIECE", "WK_SEED_LIST", "WK_LANE_CAP"):
        m = re.search(r"\b%s = (\d+)" % k, src)
        assert m and int(m.group(1)) == getattr(wc, k), k
    # the full-size seeded recipes: geometry only (nothing is materialized)
    for n in wc.names("seed"):
        c = wc.case(n)
        T = wc.SEED_BLOCKS * c.bs
        assert c.bs > wc.PAR_MAX_BS and (c.cap >= T) == (c.planned == "parallel") and c.cap < T + 8 * c.bs + (c.bs << 4), (n, c.cap)
        assert all(op[0] in ("bytes", "fill") for op in c.ops), n                     # (what the device can plant)


def test_honest_trailer_is_the_librarys(L):
    """The trailer as restated in walk_cases.trailer_bytes is byte for byte what lz4f_mi355x_appendBlockList writes."""
    for bsid in (4, 7):
        bare, honest = wc.case("trailer/bsid%d/bare" % bsid), wc.case("trailer/bsid%d/honest" % bsid)
        want = wc.materialize(honest).tobytes()
        f = want[:bare.cap]                                        # (the same layout; the payload bytes are each case's own)
        buf = ctypes.create_string_buffer(f, len(f) + 4096)
        r = L.lz4f_mi355x_appendBlockList(buf, len(f), len(f) + 4096)
        assert not L.LZ4F_isError(r) and r == len(want) and buf.raw[:r] == want, (bsid, r, len(want))
