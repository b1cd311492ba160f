"""The planted-guess corpus of the stretch self-index (tests/spx_cases.py) and its sequential model (tests/spx_model.py) on the
CPU: on every case the model's points are tokens of the plain parse (truth), start at (0, 0, 0), strictly increase and end at
(csize, count, size), and its totals are the truth's unless it declines; every case IS what its name says (its `want` predicates
over the model's verdict); every family member is there; liblz4 (the oracle) decodes every frame to the bytes the builder
recorded; and the constants and the lines of k_spx_index the model restates are the ones in csrc/decode_spx.cuh."""
import os
import re

import pytest

import oracle
import spx_cases as C
import spx_model as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lz4_frame_conduit_amd", "csrc")


@pytest.fixture(scope="module")
def corpus():
    return C.corpus()


@pytest.fixture(scope="module")
def verdicts(corpus):
    return {c.name: C.verdicts(c, fb) for c, fb, _ in corpus}


def check_points(name, payload, got, who):
    """The truth invariants on one block's verdict `got` (dict with gave_up, cnt, osz, nr, points): shared with the GPU test."""
    toks, count, size = S.truth(payload)
    if got["gave_up"]:
        assert (got["cnt"], got["osz"], got["nr"]) == (0, 0, 0), (name, who, "declined, but left counts")
        return
    pts = got["points"]
    assert len(pts) == got["nr"] + 1 and 1 <= got["nr"] <= S.MAXPT, (name, who, got["nr"], len(pts))
    assert pts[0] == (0, 0, 0), (name, who, "the first point", pts[0])
    assert pts[-1] == (len(payload), count, size), (name, who, "the last point", pts[-1], (len(payload), count, size))
    assert (got["cnt"], got["osz"]) == (count, size), (name, who, "totals", got["cnt"], got["osz"], count, size)
    by_pos = {t[0]: t for t in toks}
    for i, pt in enumerate(pts[:-1]):
        assert by_pos.get(pt[0]) == pt, (name, who, "point %d is no token of the plain parse" % i, pt, by_pos.get(pt[0]))
        assert pt[0] < pts[i + 1][0] and pt[1] < pts[i + 1][1], (name, who, "points %d and %d do not increase" % (i, i + 1), pt, pts[i + 1])


def test_model_points_are_tokens_of_the_plain_parse(corpus, verdicts):
    n = 0
    for c, fb, _ in corpus:
        comp = [(off, w) for off, w in C.payloads(fb) if not w >> 31]
        assert len(comp) == len(verdicts[c.name])
        for (off, w), m in zip(comp, verdicts[c.name]):
            check_points(c.name, fb[off:off + w], m, "model")
            n += len(m["points"])
        # without the density words the slow rule is off: the verdict the end-to-end calls (NO_DENSITY_PROBE) are held to
        if c.density is not None:
            for (off, w), m in zip(comp, C.verdicts(c, fb, None)): check_points(c.name, fb[off:off + w], m, "model, no density words")
    print("spx corpus: %d cases, %d points, %d bytes of frames" % (len(corpus), n, sum(len(f) for _, f, _ in corpus)))


def test_every_case_is_what_it_is_named_for(corpus, verdicts):
    bad = []
    for c, fb, _ in corpus:
        assert c.want and c.aim, (c.name, "a case without a want or an aim")
        m = verdicts[c.name]
        for what, fn in c.want:
            if not fn(m, c): bad.append((c.name, what, S.fates(m[0])))
        if any(x["gave_up"] for x in m) != c.declines_probe: bad.append((c.name, "declines_probe", c.declines_probe))
        if any(x["gave_up"] for x in C.verdicts(c, fb, None)) != c.declines: bad.append((c.name, "declines", c.declines))
    assert not bad, bad[:10]


def test_every_family_member_is_present(corpus):
    names = [c.name for c, _, _ in corpus]
    assert len(set(names)) == len(names), "case names repeat"
    by = {}
    for c, _, _ in corpus: by[c.family] = by.get(c.family, 0) + 1
    assert by == C.MEMBERS and set(by) == {f for f, _ in C.FAMILIES}, by
    # the declined cases are the exits' and the rescue budget's far sides, nothing else
    assert sorted(c.name for c, _, _ in corpus if c.declines) == ["exits/by_pair/longs31", "exits/hops/lane0/seqs2050", "exits/hops/lane1/seqs2050", "rescue/seqs65537"]
    assert sorted(c.name for c, _, _ in corpus if c.declines_probe and not c.declines) == ["exits/slow/under"]
    assert sorted(c.name for c, _, _ in corpus if c.density is not None) == ["exits/slow/at", "exits/slow/under"]
    sizes = sorted(len(fb) for _, fb, _ in corpus)
    assert sizes[-6] < 3 << 20 and sum(sizes) < 40 << 20, sizes[-8:]         # (only the lane-cap cases and the rescue pair are big)


def test_no_pair_but_the_planted_ones(corpus, verdicts):
    """A lane's candidates are planted bytes: a true token with 270 literals or more, or a position the case marked / a byte run
    it wrote (the decoy family's 0xFF runs).  Outside the decoy family every candidate that is no token is a lone pair."""
    for c, fb, _ in corpus:
        if c.family == "decoy": continue
        comp = [(off, w) for off, w in C.payloads(fb) if not w >> 31]
        for (off, w), m in zip(comp, verdicts[c.name]):
            toks = {t[0] for t in S.truth(fb[off:off + w])[0]}
            for l in m["lanes"]:
                if l["start"] is not None and l["cand"]: assert l["start"] in toks, (c.name, l["start"], "a lane of this family started at a pair that is no token")


def test_oracle_decodes_every_frame_to_the_recorded_bytes(corpus):
    for c, fb, out in corpus:
        ref, used = oracle.decompress_frame(fb, cap=len(out) + 64)
        assert used == len(fb) and ref == out, (c.name, "the oracle differs", used, len(fb), len(ref), len(out))
        assert 5 <= c.fr.bsid <= 7 and not c.fr.linked and not c.fr.short_mid, c.name


def test_scan_bound_follows_from_the_lane_count():
    """k_spx_index's scan stops at a + 1024 + 24 < csize.  A lane u >= 1 exists only if u * SEG + SCAN + 2048 < csize, so every KiB
    of its scan passes that bound: the scan of an existing lane is never cut short by the payload's end, which is why the corpus has
    no case on the far side of it."""
    for csize in list(range(S.SEG + S.SCAN + 2040, S.SEG + S.SCAN + 2060)) + [2 * S.SEG + S.SCAN + 2048 + d for d in (0, 1)] + [4 << 20]:
        for u in range(1, S.lanes(csize)):
            assert u * S.SEG + S.SCAN + 2048 < csize
            assert all(a + 1024 + 24 < csize for a in range(u * S.SEG, u * S.SEG + S.SCAN, 1024))
    assert S.lanes(S.SEG + S.SCAN + 2048) == 1 and S.lanes(S.SEG + S.SCAN + 2049) == 2 and S.lanes(4 << 20) == S.MAXSEG == 128


def test_model_on_hand_written_payloads():
    """step() and truth() on payloads whose answers are spelled out."""
    import lz4_grammar as G
    p = G.lz4_seq(b"abcde", 8, 3) + G.lz4_seq(b"x" * 20, 30, 5) + G.lz4_seq(b"tail!!", 0, 0)
    #      token 0x54, 5 literals, offset: 8 bytes; token 0xFF, 5, 20 literals, offset, 11: 25 bytes; token 0x60, 6 literals
    assert S.truth(p) == ([(0, 0, 0), (8, 1, 13), (33, 2, 63)], 3, 69)
    assert S.step(p, len(p), 0) == (0, 8, 13) and S.step(p, len(p), 8) == (0, 33, 50) and S.step(p, len(p), 33) == (1, 40, 6)
    assert S.step(p, len(p), 34)[0] == 2 and S.step(p, len(p), 40)[0] == 2            # (a guessed byte; the payload's end)
    assert S.step(p, len(p), 0, (1 << 23) - 12)[0] == 2 and S.step(p, len(p), 0, (1 << 23) - 13)[0] == 0
    m = S.model(p)
    assert (m["gave_up"], m["cnt"], m["osz"], m["nr"], m["points"]) == (False, 3, 69, 1, [(0, 0, 0), (40, 3, 69)])
    assert S.model(p, (0, 100))["gave_up"] and not S.model(p, (1, 100))["gave_up"] and S.model(b"")["gave_up"]
    assert list(S.pairs(bytes([0xF0, 0xFF, 0xFF, 0x0F, 0xFF, 0xE0, 0xFF]))) == [True, True, False, False, False, False, False]


def test_constants_are_the_kernels():
    with open(os.path.join(CSRC, "decode_spx.cuh")) as f: text = f.read()
    lines = [l for l in text.splitlines() if "constexpr" in l or "#define" in l]
    for name, want in S.CONSTANTS.items():
        got = [m.group(1) for l in lines for m in re.finditer(r"\b%s\s*(?:=|\s)\s*(0x[0-9A-Fa-f]+|\d+u? << \d+|\d+)u?\b" % name, l)]
        assert got and all(eval(g.replace("u", "")) == want for g in got), (name, want, got)
    assert "SPX_SEG = SPX_SEG_BYTES" in text and "SPX_MAXSEG = (4u << 20) / SPX_SEG" in text
    for expr in S.SOURCE_LINES:
        assert expr in text, (expr, "the kernel's text changed: look at the model's restatement of it")
