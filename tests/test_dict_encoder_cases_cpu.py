"""The planted dictionary corpus (dict_encoder_cases.py) and its fixture (tests/golden/dict_planted.json, minted from liblz4 by
tools/mint_dict_planted.py): the cases are what they say, liblz4's chain search writes the planted parse, and the checkers the GPU
tests rely on flag what they are there to flag.  No GPU, no liblz4."""
import numpy as np
import pytest

import dict_cases as dc
import dict_encoder_cases as de
import encoder_cases as ec
import lz4_writer_rules as wr


@pytest.fixture(scope="module")
def fx():
    return de.load_fixture()


def test_fixture_is_the_minted_one(fx):
    de.check_sha(fx)
    assert set(fx["dicts"]) == set(de.DICT_LEN)
    for c in de.corpus():
        assert set(c.framings) <= set(fx["cases"][c.name]) and fx["cases"][c.name]["dict"] == c.dname and fx["cases"][c.name]["len"] == len(c.data)


def test_dictionaries_and_shapes():
    assert {n: len(de.dictionary(n)) for n in de.DICT_LEN} == de.DICT_LEN
    assert {c.fam for c in de.corpus()} == set(de.FAMILIES)
    for c in de.corpus():
        assert set(c.framings) <= set(de.FRAMINGS)
        assert len(c.data) <= (132 << 10 if c.fam in ("block2", "chunk/second") else 66 << 10), c.name
    by = lambda fam: [c for c in de.corpus() if c.fam == fam]
    assert {(c.dname, p) for c in by("reach/far") for p in c.plants()} == {(d, (x, M, 65535)) for d in ("k64k-1", "k64k", "k70k") for M in (40, 600) for x in (1, 100)}
    assert {p[2] for c in by("reach/far") + by("mpos0") for p in c.plants()} >= {65535}
    assert all(c.build()[2] and not c.expected(fr) for c in by("reach/ghost") for fr in c.framings)
    for c in by("reach/first"):
        (x, M, dist), = c.plants()[:1]
        assert dist == x + c.DL and M == min(c.DL, 40) and x in (1, 100), c.name
    for c in by("reach/last"):
        x, M, dist = c.plants()[0]
        assert dist == x + M and M in (4, 5, 40), c.name                       # the source ends with the dictionary
    for c in by("mpos0"):
        assert c.expected("i64")[0][0] == 0 and c.expected("i64")[0][3] == 0, c.name


def test_no_case_has_flaws():
    for c in de.corpus():
        concat, plants, ghosts = c.build()
        assert concat[:c.DL] == de.dictionary(c.dname), c.name                 # frozen
        assert c.flaws(np.frombuffer(concat, np.uint8), plants, ghosts) == [], c.name


def test_the_flaw_checks_see_across_the_seam():
    """A window of the input that the dictionary holds too, and a plant that could go on: the checks are the concatenation's."""
    c = next(c for c in de.corpus() if c.name == "reach/last/k1k/M40")
    concat, plants, ghosts = c.build()
    d = np.frombuffer(concat, np.uint8).copy()
    d[c.DL + 70:c.DL + 74] = d[500:504]
    assert any("occurs before" in what for what, _ in c.flaws(d, plants, ghosts))
    d = np.frombuffer(concat, np.uint8).copy()
    pos, M, _ = plants[0]
    d[pos + M] = d[c.DL]                                                        # the byte behind the plant: the input's first, behind the seam
    assert any("extends forwards" in what for what, _ in c.flaws(d, plants, ghosts))


def test_planted_parse_decodes_to_the_input():
    n = 0
    for c, fr in de.pairs():
        frame = de.planted_frame(c, fr)
        v = dc.model_decode(frame, de.dictionary(c.dname))
        assert v.ok and v.out == c.data and v.consumed == len(frame), (c.name, fr, v.why)
        assert wr.audit(frame, c.data, ec.FRAMINGS[fr], dict_len=c.D) == [], (c.name, fr)
        seqs = de.frame_seqs(frame)
        assert de.parse_of(c, fr, seqs) == c.expected(fr), (c.name, fr)
        assert de.straddlers(seqs, len(c.data), ec.BS[fr], ec.FRAMINGS[fr]["linked"]) == [], (c.name, fr)
        assert de.literal_everywhere(seqs, len(c.data), ec.BS[fr], c.ghosts(fr)), (c.name, fr)
        # the helper's merge is lz4_writer_rules.matches'
        assert de.rows(seqs, len(c.data), ec.BS[fr], True) == [tuple(r) for r in wr.matches(frame).tolist()], (c.name, fr)
        n += bool(c.expected(fr))
    assert n >= 150


def test_ghosts_are_out_of_reach():
    seen = 0
    for c in de.corpus():
        for pos, M, dist in c.build()[2]:
            assert dist > 65535 or pos - dist < c.DL - c.D, c.name             # too far, or in front of the bytes that count
            seen += 1
        for fr in c.framings:
            for (x, M, dist), ok in c._placed(fr):
                if not ok: assert dist > 65535, (c.name, fr)
    assert seen >= 13
    front = next(c for c in de.corpus() if c.name == "reach/ghost/k70k/front")
    (pos, M, dist), = front.build()[2]
    assert pos - dist == 100 and pos - dist + M <= front.DL - front.D and dist == 100 + 70000 - 100


def test_framings_place_the_dictionary():
    """block2's plant: the dictionary in front of an independent frame's second block, out of reach in a linked frame."""
    c = next(c for c in de.corpus() if c.name == "block2/k1k")
    assert c.expected("i64")[-1] == (65536 + 100, 40, 100 + 1024 - 500, 100)
    for fr in ("l64", "l256"):
        assert all(r[0] < 65536 for r in c.expected(fr)) and c.ghosts(fr) == [(65636, 40)]
    s = next(c for c in de.corpus() if c.name == "chunk/second/k1k")
    assert s.framings == ("l64", "l256") and all(s.ghosts(fr) == [(65546, 40)] for fr in s.framings)
    r = next(c for c in de.corpus() if c.name == "chunk/last_reach/k1k")
    assert r.expected("l256")[-1] == (65494, 40, 65535, 30) and r.expected("i64")[-1] == (65494, 65536 - 5 - 65494, 65535, 30)
    assert r.expected("i64")[-1][0] <= 65536 - 12


def test_liblz4_writes_the_planted_parse(fx):
    """The caps of the fixture: at least 9 in 10 of all pairs forced, and every pair of the reach and seam/cross families."""
    pairs = de.pairs()
    forced = {(c.name, fr) for c, fr in pairs if de.is_forced(fx, c, fr)}
    print("%d of %d (case, framing) pairs are forced" % (len(forced), len(pairs)))
    assert len(forced) * 10 >= len(pairs) * 9
    loose = [(c.name, fr) for c, fr in pairs if c.fam in de.MUST_BE_FORCED and (c.name, fr) not in forced]
    assert not loose, loose
    for fam in de.FAMILIES:
        assert any(c.fam == fam and (c.name, fr) in forced for c, fr in pairs), fam
    # the figures liblz4 was seen to write
    S = lambda name, fr, lv: [tuple(s) for s in fx["cases"][name][fr]["seqs%d" % lv][0]]
    for dn in ("k64k-1", "k64k", "k70k"):
        assert S("reach/far/%s/M40/x100" % dn, "i64", 9)[0] == (100, 40, 65535) and S("reach/far/%s/M600/x100" % dn, "l64", 9)[0] == (100, 600, 65535)
        assert fx["cases"]["reach/ghost/%s/M600/x100" % dn]["i64"]["seqs9"] == [None]                   # 65536 back: stored
    assert S("seam/cross/k1k/K30", "i64", 9)[:2] == [(50, 40, 90), (0, 30, 90)]
    assert S("seam/cross/k1k/K30", "i64", 0)[:1] == [(50, 70, 90)]
    assert S("pick/k1k", "i64", 9)[1] == (40, 60, 1024 - 200 + 78)


def test_the_no_straddle_check_bites(fx):
    """liblz4's fast finder lets a match run across the seam; the check the device's frames are held to flags exactly that."""
    for dn in ("k64", "k1k"):
        c = next(c for c in de.corpus() if c.name == "seam/cross/%s/K30" % dn)
        for fr in c.framings:
            n, bs, linked = len(c.data), ec.BS[fr], ec.FRAMINGS[fr]["linked"]
            assert de.straddlers(fx["cases"][c.name][fr]["seqs0"], n, bs, linked) == [(50, 70, 90)], (dn, fr)
            assert de.straddlers(fx["cases"][c.name][fr]["seqs9"], n, bs, linked) == [], (dn, fr)
    # an overlapping match is judged by where it starts reading and its first `off` bytes
    assert de.straddlers([[(10, 50, 12), (5, 0, 0)]], 65, 65536, False) == [(10, 50, 12)]         # 2 bytes of dictionary, then its own output
    assert de.straddlers([[(10, 50, 10), (5, 0, 0)]], 65, 65536, False) == []                     # begins at the input's first byte
    assert de.straddlers([[(10, 50, 3), (5, 0, 0)]], 65, 65536, False) == []
    assert de.straddlers([[(0, 40, 40), (5, 0, 0)]], 45, 65536, False) == []                      # ends at the dictionary's last byte
    # an independent frame's second block has the dictionary in front of it, a linked frame's has the first block
    two = [[(65536, 0, 0)], [(10, 50, 12), (5, 0, 0)]]
    assert de.straddlers(two, 65536 + 65, 65536, False) == [(65546, 50, 12)] and de.straddlers(two, 65536 + 65, 65536, True) == []


def test_the_ghost_check_bites(fx):
    c = next(c for c in de.corpus() if c.name == "block2/k1k")
    n = len(c.data)
    assert de.literal_everywhere(fx["cases"][c.name]["l64"]["seqs9"], n, 65536, c.ghosts("l64"))
    assert not de.literal_everywhere(fx["cases"][c.name]["i64"]["seqs9"], n, 65536, c.ghosts("l64"))   # (where it is a plant, a match covers it)


@pytest.mark.parametrize("mode", dc.MODES)
def test_offset_reach_counts_the_dictionary(mode):
    """dict_cases' planted frames: an offset to the dictionary's first byte is within reach, one byte more is not - and without
    dict_len both are out of reach, as every verdict of the audit so far has it."""
    for dname in ("d1k", "d3"):
        d = dc.dictionary(dname)
        frames = {n: f for n, m, f in dc.planted(dname) if m == mode}
        plus1, exact = frames["off_plus1"], frames["off_exact"]
        out = dc.model_decode(exact, d).out
        assert "offset-reach" in wr.rules(wr.audit(plus1, out, dict_len=len(d)))
        assert wr.audit(exact, out, dict_len=len(d)) == []
        assert "offset-reach" in wr.rules(wr.audit(exact, out))
        assert "offset-reach" in wr.rules(wr.audit(exact, out, dict_len=len(d) - 1))
    if mode == "linked":                                                        # behind 64 KiB of output no offset reaches a dictionary
        d = dc.dictionary("d1k")
        far = {n: f for n, m, f in dc.planted("d1k") if m == mode}["third_block_far"]
        out = dc.model_decode(far, d).out                                       # (its flushed short block breaks block-length, with and without)
        assert wr.audit(far, out, dict_len=len(d)) == wr.audit(far, out) and "offset-reach" not in wr.rules(wr.audit(far, out))
