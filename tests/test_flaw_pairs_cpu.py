"""The two-flaw corpus (tests/flaw_pairs.py) against liblz4's recorded answers (tests/golden/flaw_pairs.json), without a GPU:
the frames are the minted ones, the oracle answers as liblz4 does, the first flaw decides in every pair, the pairs can tell the
orders apart, the model of the written order is the oracle's wherever one flaw leaves no order to choose, and the comparison
the GPU tests use catches a chooser that picks wrongly."""
import collections

import pytest

import flaw_pairs as fp


@pytest.fixture(scope="module")
def fx():
    return fp.load_fixture()["cases"]


@pytest.fixture(scope="module")
def cases():
    return fp.cases()


def test_the_regenerated_frames_are_the_minted_ones(fx, cases):
    assert [c.name for c in cases] == list(fp.names()) and sorted(fx) == sorted(fp.names())
    for c in cases:
        assert fp.sha(c.frame) == fx[c.name]["frame_sha256"], c.name
        assert c.frame[4] == (0x74 if c.mode == "indep" else 0x54) | (8 if ("csize", None) in c.flaws else 0), c.name      # FLG: the mode is the header's


def test_the_corpus_has_the_cases_the_orders_differ_on(cases):
    by = collections.Counter((c.shape, c.mode) for c in cases if fp.block_pair(c))
    for mode in fp.MODES:
        assert by["short5", mode] == by["full3s", mode] == by["full3d", mode] == 25
        assert (by["edge64", mode], by["edge65", mode], by["edge130", mode]) == (4, 4, 12)
        have = {c.name for c in cases if c.mode == mode}
        for a in fp.BLOCK_ATOMS:
            for f in ("trunc.pay@3", "trunc.bck@3", "trunc.word@3", "trunc.end", "trunc.cck", "room@3", "csize", "cck"):
                assert "short5/%s/%s@1+%s" % (mode, a, f) in have
            for f in ("trunc.pay@1", "trunc.bck@1", "trunc.word@1", "room@1"):
                assert "short5/%s/%s+%s@3" % (mode, f, a) in have
        for nm in ("bck@1+cut@1", "bck@1+over@1", "csize+cck", "room@3+cck", "trunc.pay@3+csize", "clean"):
            assert "short5/%s/%s" % (mode, nm) in have
    for c in cases:                                                   # every pair comes with its two flaws alone
        if fp.is_pair(c):
            assert all(p in fp.names() for p in fp.parts(c)), c.name
    assert {fp.SHAPES[s][0] for s in ("edge64", "edge65", "edge130")} == {64, 65, 130}


def test_whole_and_pieces_are_one_answer(fx, cases):
    for c in cases:
        assert fp.ref_verdict(fx[c.name]["once"]) == fp.ref_verdict(fx[c.name]["pieces"]), c.name


def test_the_oracle_answers_as_liblz4(fx, cases):
    bad = [(c.name, fp.oracle_verdict(c), fp.ref_verdict(fx[c.name]["once"])) for c in cases
           if fp.oracle_verdict(c) != fp.ref_verdict(fx[c.name]["once"])]
    assert not bad, (len(bad), bad[:20])
    assert sum(fp.ref_verdict(fx[c.name]["once"]).startswith("OK:") for c in cases) == 12      # the clean frames, and nothing else


def test_the_first_flaw_decides(fx, cases):
    """The corpus bites: liblz4's answer to a pair is its answer to the pair's first flaw alone."""
    n = 0
    for c in cases:
        if fp.is_pair(c):
            first, _ = fp.parts(c)
            assert fp.ref_verdict(fx[c.name]["once"]) == fp.ref_verdict(fx[first]["once"]), c.name
            assert not fp.ref_verdict(fx[first]["once"]).startswith("OK:"), first
            n += 1
    assert n >= 2 * (25 + 2 + 40 + 20 + 3 + 50 + 20)


def test_the_pairs_tell_the_orders_apart(fx, cases):
    """At least 16 of the 25 ordered block-atom pairs of a shape have two flaws that liblz4 names differently (cut and over are one
    name, word and stored_over another: 9 pairs cannot differ)."""
    differ = collections.Counter()
    for c in cases:
        if fp.block_pair(c):
            a, b = fp.parts(c)
            differ[c.shape, c.mode] += fp.ref_verdict(fx[a]["once"]) != fp.ref_verdict(fx[b]["once"])
    for sh in ("short5", "full3s", "full3d"):
        for mode in fp.MODES:
            assert differ[sh, mode] >= 16, (sh, mode, differ[sh, mode])
    for sh, n in (("edge64", 4), ("edge65", 4), ("edge130", 12)):      # bck and cut in both orders: every one of them differs
        for mode in fp.MODES:
            assert differ[sh, mode] == n, (sh, mode)


WORD = {fp.GENERIC: "ERROR_blockFailed", fp.MAXBLOCK: "ERROR_maxBlockSize_invalid", fp.BLOCKCK: "ERROR_blockChecksum_invalid",
        fp.DSTSMALL: "STALL_room", fp.INCOMPLETE: "STALL_input", fp.FRAMESIZE: "ERROR_frameSize_wrong", fp.CONTENTCK: "ERROR_contentChecksum_invalid"}


def test_the_model_is_the_oracle_where_one_flaw_leaves_no_choice(fx, cases):
    """The written order puts the walk in front of the blocks, which liblz4 does not: with two flaws the two may differ, with one
    they may not.  (Back-to-back placement: the oracle's; the provisional places are the device calls' own rule.)"""
    for c in cases:
        if len(c.flaws) <= 1:
            win = fp.room_window(c, False) if c.room is not None else fp.ample(c)
            st, bad = fp.one_shot_verdict(c, win, placed=False)
            want = fp.ref_verdict(fx[c.name]["once"])
            assert (st == 0 and want.startswith("OK:")) or WORD.get(st) == want, (c.name, st, want)
            blocks = [b for a, b in c.flaws if a in ("cut", "over", "bck", "room")]      # (the flaws a block is judged for)
            assert bad == (blocks[0] if blocks else fp.NONE), (c.name, bad)


def test_a_wrong_chooser_is_caught(cases):
    """The GPU tests' comparison, fed by two deliberately wrong rules: each must be reported, and the right one must not."""
    def rows(rule):
        return [(c.name, "model:" + rule, fp.one_shot_verdict(c, w, rule=rule), fp.one_shot_verdict(c, w), c.mode == "linked")
                for c in cases for w in fp.windows(c, True)]
    assert fp.disagreements(rows("first")) == []
    last = fp.disagreements(rows("last"))
    assert any("cut@1+bck@3" in name for name, _, _, _ in last) and len(last) >= 100, len(last)
    dec = fp.disagreements(rows("decode_first"))
    assert dec and all("bck@1+cut@1" in name or "bck@1+over@1" in name for name, _, _, _ in dec), dec[:5]
    # the stated exception lets a later block of a linked frame pass, never another status or an earlier block
    assert fp.disagreements([("x", "e", (1, 3), (1, 1), True)]) == []
    assert fp.disagreements([("x", "e", (7, 3), (1, 1), True), ("x", "e", (1, 0), (1, 1), True), ("x", "e", (1, 3), (1, 1), False)]) != []
    assert len(fp.disagreements([("x", "e", (7, 3), (1, 1), True), ("x", "e", (1, 0), (1, 1), True), ("x", "e", (1, 3), (1, 1), False)])) == 3
