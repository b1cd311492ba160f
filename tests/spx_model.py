"""The stretch self-index (csrc/decode_spx.cuh, k_spx_index) as two plain sequential programs (test helper, not a test module).

truth(payload)   the lengths-only parse of one LZ4 block, written from the block format alone: every token's (payload position,
                 sequence number, output position), the sequence count and the decoded size.  It knows nothing of lanes.
model(payload, density=None)
                 a restatement of k_spx_index as its header and comments define it, one step after the other: spx_lanes; the
                 pair scan KiB by KiB (its `a + 1024 + 24 < csize` bound, stopping at the first KiB that shows a pair, at most
                 SPX_CAND candidates in position order); spx_likely_token; each lane's `stop`; the walk with its notes every
                 SPX_SUB_STRIDE hops and the keep-odd compaction that doubles the stride; the `slow`, `by_pair` and
                 SPX_LANE_HOPS exits; the stitch with its skip conditions, the SPX_RESCUE budget and the decline on a true lane
                 without a landing; the order of the points in T.  `density` is (not_dense, bytes_per_seq), the two words of
                 k_density_probe the kernel reads, or None for no only_if (LZ4F_MI355X_NO_DENSITY_PROBE).
The two share step() only in the model: truth() has its own loop.  tests/test_spx_model_cpu.py holds the model's points to the
truth on every case of tests/spx_cases.py and reads CONSTANTS back from decode_spx.cuh; tests/test_gpu_spx_index.py holds the
kernel to both.

A sequence as the walk sees it (spx_step): lengths only, offsets are not looked at; 2 = not a sequence this payload can hold (a
length byte beyond the payload, 2^24 literals or more, literals that end neither 8 bytes in front of the payload's end nor exactly
on it, an output beyond 2^23), 1 = the block's last sequence, 0 = went on.  Bytes behind the payload never change a verdict: the
kernel's wide loads may see them, every use of them is behind a bound that this restatement applies to the payload alone.
"""
from __future__ import annotations

import numpy as np

CONSTANTS = dict(SPX_SEG_BYTES=32768, SPX_SCAN=8192, SPX_CAND=6, SPX_LANE_HOPS=2048, SPX_RESCUE=1 << 16, SPX_SUB=8, SPX_SUB_STRIDE=16)
SEG, SCAN, CAND = CONSTANTS["SPX_SEG_BYTES"], CONSTANTS["SPX_SCAN"], CONSTANTS["SPX_CAND"]
LANE_HOPS, RESCUE, SUB, SUB_STRIDE = CONSTANTS["SPX_LANE_HOPS"], CONSTANTS["SPX_RESCUE"], CONSTANTS["SPX_SUB"], CONSTANTS["SPX_SUB_STRIDE"]
MAXSEG = (4 << 20) // SEG
MAXPT = MAXSEG * (SUB + 1)
NONE = 0xFFFFFFFF
# text of the kernel the model restates (file decode_spx.cuh): the CPU test looks for each
SOURCE_LINES = [
    "if (csize <= SPX_SEG + SPX_SCAN + 2048u) return 1u;",
    "const uint32_t n = (csize - SPX_SCAN - 2048u - 1u) / SPX_SEG + 1u;",
    "for (uint32_t a = from; a < from + SPX_SCAN && a + 1024u + 24u < csize && n == 0; a += 1024u) {",
    "if (r == 0 && c.pos + 2 < csize) {",
    "if (s_g[k] != SPX_NONE && s_g[k] > s_g[u]) { stop = s_g[k]; break; }",
    "const uint32_t slow = (u && s_g[u] == u * SPX_SEG && only_if) ? only_if[1] / 8u : 0u;",
    "const bool by_pair = u && s_g[u] != u * SPX_SEG;",
    "if (hops && hops % sub_stride == 0) {",
    "s_sub[u][i] = s_sub[u][2 * i + 1]; nsub = SPX_SUB / 2; sub_stride *= 2;",
    "if ((hops & 63u) == 63u) {",
    "if (slow && c.pos - s_g[u] < hops * slow) break;",
    "if (by_pair && longs * 2u < hops) break;",
    "if (hops > SPX_LANE_HOPS) break;",
    "if (kn < nl && (s_g[kn] == SPX_NONE || s_g[kn] < nx.pos)) { kn++; continue; }",
    "if (++rescue > SPX_RESCUE) { bad = true; break; }",
    "else { bad = true; break; }",
    "constexpr uint32_t SPX_MAXPT = SPX_MAXSEG * (SPX_SUB + 1);",
]


# ------------------------------------------------------------------------------------------------------------------------
def truth(payload: bytes):
    """(tokens, count, size): tokens[i] = (pos, seq, out) of sequence i - its token's payload position, its number, the output
    position in front of its literals.  Of the format's rules only what parsing needs: the sequence whose literals reach the
    payload's end is the last one and has no match, every other one has an offset and its match-length bytes inside the payload."""
    p, n = payload, len(payload)
    assert n > 0
    toks, pos, out = [], 0, 0
    while True:
        toks.append((pos, len(toks), out))
        t = p[pos]; pos += 1
        lit = t >> 4
        if lit == 15:
            while True:
                v = p[pos]; pos += 1; lit += v
                if v != 255: break
        pos += lit; out += lit
        assert pos <= n, "literals run past the payload"
        if pos == n: break
        assert pos + 2 <= n, "an offset cut by the payload's end"
        pos += 2
        ml = t & 15
        if ml == 15:
            while True:
                v = p[pos]; pos += 1; ml += v
                if v != 255: break
        out += ml + 4
        assert pos < n, "a match is the payload's last thing"
    return toks, len(toks), out


# ------------------------------------------------------------------------------------------------------------------------
def lanes(csize: int) -> int:
    """spx_lanes"""
    if csize <= SEG + SCAN + 2048: return 1
    return min((csize - SCAN - 2048 - 1) // SEG + 1, MAXSEG)


def step(p: bytes, csize: int, pos: int, out: int = 0):
    """spx_step at `pos` with `out` output bytes counted so far: (r, next position, output bytes of the sequence)."""
    if pos >= csize: return 2, pos, 0
    t = p[pos]
    lit, q = t >> 4, pos + 1
    if lit == 15:
        while True:
            if q >= csize: return 2, pos, 0
            v = p[q]; q += 1; lit += v
            if v != 255: break
            if lit >= 1 << 24: return 2, pos, 0
    if q > csize or lit >= 1 << 24: return 2, pos, 0
    left = csize - q
    if lit + 8 > left:
        return (1, csize, lit) if lit == left else (2, pos, 0)
    q += lit + 2
    ml = t & 15
    if ml == 15:
        while True:
            if q >= csize: return 2, pos, 0
            v = p[q]; q += 1; ml += v
            if v != 255: break
            if ml > 1 << 24: return 2, pos, 0
    if out + lit + ml + 4 > 1 << 23: return 2, pos, 0
    return 0, q, lit + ml + 4


def pairs(payload: bytes):
    """mask[i]: byte i is 0xF? and byte i + 1 is 0xFF"""
    a = np.frombuffer(payload, dtype=np.uint8)
    m = np.zeros(len(a), dtype=bool)
    m[:-1] = ((a[:-1] & 0xF0) == 0xF0) & (a[1:] == 0xFF)
    return m


def candidates(mask, csize: int, u: int):
    """The pair scan of lane u's segment: (candidate positions, KiBs read)."""
    frm, a, kib = u * SEG, u * SEG, 0
    while a < frm + SCAN and a + 1024 + 24 < csize:
        kib += 1
        hit = np.flatnonzero(mask[a:a + 1024])
        if len(hit): return [a + int(i) for i in hit[:CAND]], kib
        a += 1024
    return [], kib


def likely_token(p: bytes, csize: int, at: int) -> bool:
    r, pos, _ = step(p, csize, at)
    if r == 1: return True
    return r == 0 and pos + 2 < csize and (p[pos] & 0xF0) == 0xF0 and p[pos + 1] == 0xFF


def model(payload: bytes, density=None):
    """k_spx_index on one compressed block's payload -> dict: gave_up, stitched (stretches the stitching thread walked), cnt,
    osz, nr, points [(pos, seq, out)] (nr + 1 of them; none when it declines), and per lane `lanes`[u] = dict(start (None: stays
    out), cand, kib, fate, hops, landing, true): fate is one of out / landed / ended / slow / by_pair / hops / ran_into;
    true: the stitch found the lane's start on the true chain."""
    p, csize = payload, len(payload)
    declined = dict(gave_up=True, stitched=0, cnt=0, osz=0, nr=0, points=[], lanes=[])
    if density is not None and density[0] == 0: return declined
    if csize == 0: return declined
    nl = lanes(csize)
    mask = pairs(p)
    L = []
    # ---- every lane's start
    for u in range(nl):
        if u == 0: L.append(dict(start=0, cand=[], kib=0)); continue
        cand, kib = candidates(mask, csize, u)
        g = None if cand else u * SEG
        for at in cand:
            if likely_token(p, csize, at): g = at; break
        L.append(dict(start=g, cand=cand, kib=kib))
    # ---- every lane's walk
    for u, l in enumerate(L):
        l.update(fate="out", hops=0, landing=None, ended=False, notes=[], true=False)
        g = l["start"]
        if g is None: continue
        stop = NONE
        for k in range(u + 1, nl):
            if L[k]["start"] is not None and L[k]["start"] > g: stop = L[k]["start"]; break
        slow = density[1] // 8 if (u and g == u * SEG and density is not None) else 0
        by_pair = bool(u) and g != u * SEG
        pos, seq, out = g, 0, 0
        longs, stride, notes, hops = 0, SUB_STRIDE, [], 0
        while True:
            if pos >= stop: l.update(fate="landed", landing=(pos, seq, out)); break
            if hops and hops % stride == 0:
                if len(notes) == SUB: notes = notes[1::2]; stride *= 2
                if hops % stride == 0: notes.append((pos, seq, out))
            if hops & 63 == 63:
                if slow and pos - g < hops * slow: l["fate"] = "slow"; break
                if by_pair and longs * 2 < hops: l["fate"] = "by_pair"; break
            if pos < csize and (p[pos] & 0xF0) == 0xF0: longs += 1
            if hops > LANE_HOPS: l["fate"] = "hops"; break
            r, pos, d = step(p, csize, pos, out)
            if r == 2: l["fate"] = "ran_into"; break
            seq += 1; out += d
            if r == 1: l.update(fate="ended", landing=(pos, seq, out), ended=True); break
            hops += 1
        l["hops"] = hops
        l["notes"] = notes if l["landing"] is not None else []
    # ---- the stitch
    res = dict(gave_up=False, stitched=0, cnt=0, osz=0, nr=0, points=[], lanes=L)
    k, rescue, bad, cur, pts, total = 0, 0, False, (0, 0, 0), [], None
    g_of = lambda i: NONE if L[i]["start"] is None else L[i]["start"]
    while True:
        l = L[k]
        l["true"] = True
        pts.append((g_of(k), cur[1], cur[2]))
        pts += [(a, cur[1] + s, cur[2] + o) for a, s, o in l["notes"]]
        if l["landing"] is None: bad = True; break
        nx = (l["landing"][0], cur[1] + l["landing"][1], cur[2] + l["landing"][2])
        ended = l["ended"]
        kn = k + 1
        while not ended and not (kn < nl and g_of(kn) == nx[0]):
            if kn < nl and (g_of(kn) == NONE or g_of(kn) < nx[0]): kn += 1; continue
            stop = g_of(kn) if kn < nl else NONE
            res["stitched"] += 1
            pos, seq, out = nx
            while True:
                if pos >= stop: break
                rescue += 1
                if rescue > RESCUE: bad = True; break
                r, pos, d = step(p, csize, pos, out)
                if r == 2: bad = True; break
                seq += 1; out += d
                if r == 1: ended = True; break
            if bad: break
            nx = (pos, seq, out)
        if bad: break
        if ended:
            if nx[0] != csize: bad = True; break
            total = nx; break
        k, cur = kn, nx
    res["rescue"] = rescue
    if bad or total is None or total[1] == 0:
        res["gave_up"] = True
        return res
    pts.append((csize, total[1], total[2]))
    res.update(cnt=total[1], osz=total[2], nr=len(pts) - 1, points=pts)
    return res


def fates(m) -> str:
    """The lanes of a verdict in a line, for failure messages."""
    return " ".join("%d:%s%s@%s" % (u, l["fate"], "*" if l["true"] else "", l["start"]) for u, l in enumerate(m["lanes"]))
