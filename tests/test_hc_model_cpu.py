"""The sequential model of the hash-chain encoder (hc_model.py) and its cases (hc_choice_cases.py), held to what does not depend
on either: a search without hash or chain, the block format's decoder and writer rules, and - case by case - the condition that the
decision a case is named for changes its parse.  tests/test_gpu_hc_model.py then holds the kernels to the model."""
import numpy as np
import pytest

import oracle
import hc_choice_cases as cc
import hc_model as hm
import lz4_writer_rules as wr

SMALL = 16 << 10


def header(fr: str) -> bytes:
    f = cc.FRAMINGS[fr]
    return oracle.header_bytes(oracle.mkprefs(bsid=f["bsid"], indep=0 if f["linked"] else 1))


def seqs(P) -> list:
    return [B["seqs"] for B in P.blocks]


def in_dictionary(P) -> bool:
    return any(src < win.seam for _, _, _, _, ev, win in P.chunks for _, _, src in ev)


def test_levels():
    assert [hm.level_params(l) for l in (3, 5, 6, 12, 13, 100)] == [(32, 1), (64, 1), (256, 2), (8192, 2), (8192, 2), (8192, 2)]
    assert [hm.level_params(l)[0] for l in range(3, 13)] == [32, 48, 64, 256, 384, 512, 1024, 2048, 4096, 8192]


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_search_is_the_hash_free_definition(fam):
    """Every case whose windows are under 16 KiB: with unlimited attempts each position's (length, offset) is the longest match
    among all earlier positions within reach, the nearest among equals - found without a hash."""
    n = 0
    for c in cc.corpus():
        if c.fam != fam: continue
        for _, _, win in c.model(c.framings[0]).windows:
            if len(win.w) >= SMALL: continue
            L, O, _ = win.search([hm.UNLIMITED])[hm.UNLIMITED]
            EL, EO = hm.exhaustive(win)
            bad = np.flatnonzero((L != EL) | (O != EO))
            assert len(bad) == 0, (c.name, int(bad[0]), int(L[bad[0]]), int(O[bad[0]]), int(EL[bad[0]]), int(EO[bad[0]]))
            n += 1
    assert n or fam == "text", fam


@pytest.mark.parametrize("fr", cc.ALL)
@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_model_writes_a_valid_parse(fam, fr):
    """The model's records, written out as blocks: the oracle's block decoder gives the input back, no writer rule is broken, and
    the rows and the size the model states are those of the frame."""
    f = cc.FRAMINGS[fr]
    for c in cc.select(fam, fr):
        data, d = c.data, (c.dictionary or b"")
        tail = d[-65536:] if len(d) >= 4 else b""
        for lvl in c.levels:
            P = c.parse(fr, lvl)
            for k, B in enumerate(P.blocks):
                if B["stored"]: continue
                hist = (tail + data[:B["start"]])[-65536:] if f["linked"] else tail
                got = oracle.decompress_block(P.payload(k), B["blen"], hist)
                assert got == data[B["start"]:B["start"] + B["blen"]], (c.name, lvl, k)
            frame = P.frame(header(fr))
            assert len(frame) == P.frame_size(), (c.name, lvl)
            assert wr.audit(frame, data, dict(bsid=f["bsid"], linked=f["linked"], bck=False, cck=False), dict_len=len(tail)) == [], (c.name, lvl)
            assert wr.matches(frame).tolist() == P.rows.tolist(), (c.name, lvl)


def test_no_block_is_stored_outside_raw():
    """... but for blocks of 13 bytes and less, which have no room for a match that pays (end/)."""
    for c in cc.corpus():
        if c.fam == "raw": continue
        for fr in c.framings:
            for B in c.parse(fr, c.levels[0]).blocks:
                assert not B["stored"] or (c.fam == "end" and B["blen"] <= 13), (c.name, fr, B["start"], B["blen"], B["size"])


# ---------------------------------------------------------------------------------------------------------------------
def test_attempts_cases_decide():
    for c in cc.select("attempts", "i64"):
        if c.name == "attempts/ladder": continue
        k = c.meta["k"]
        assert k in (c.attempts - 1, c.attempts, c.attempts + 1), c.name
        P = {a: c.model("i64").parse(9, attempts=a) for a in (k - 1, k, k + 1) if a >= 1}
        p = c.meta["p"]
        found = {a: any(r[0] == p and r[1] == 40 for r in v.rows.tolist()) for a, v in P.items()}
        assert found == {a: a >= k for a in P}, (c.name, found)
        if k >= 2: assert seqs(P[k - 1]) != seqs(P[k]), c.name


def test_ladder_gives_ten_parses():
    c = [c for c in cc.corpus() if c.name == "attempts/ladder"][0]
    assert c.levels == tuple(range(3, 14))
    c.model("i64").windows[0][2].search(list(hm.ATTEMPTS))
    P = [seqs(c.parse("i64", lvl)) for lvl in range(3, 14)]
    assert all(P[i] != P[j] for i in range(10) for j in range(i))
    assert P[10] == P[9]


def test_lazy_cases_decide():
    want = {"lazy/second_longer_by_2": True}
    for c in cc.select("lazy", "i64"):
        for fr in c.framings:
            one, two = c.parse(fr, 9, lazy=1), c.parse(fr, 9, lazy=2)
            assert (seqs(one) != seqs(two)) == want.get(c.name, False) == c.meta["lazy_differs"], (c.name, fr)
    by = {c.name: c for c in cc.select("lazy", "i64")}
    taken = lambda c, lazy: [r[0] - c.meta["p"] for r in c.parse("i64", 9, lazy=lazy).rows.tolist() if 0 <= r[0] - c.meta["p"] < 200]
    assert taken(by["lazy/next_longer_by_1"], 1)[0] == 1 and taken(by["lazy/next_equal"], 1)[0] == 0
    assert taken(by["lazy/second_longer_by_2"], 2)[0] == 2 and taken(by["lazy/second_longer_by_2"], 1)[0] == 0
    assert taken(by["lazy/second_longer_by_1"], 2)[0] == 0
    assert taken(by["lazy/stairs_over_a_reload"], 1)[0] == 70 and taken(by["lazy/stairs_over_a_batch"], 1)[0] == 70
    p = by["lazy/stairs_over_a_batch"].meta["p"]
    assert p // cc.HC_T < (p + 70) // cc.HC_T
    for name in ("lazy/stairs_over_a_reload", "lazy/stairs_over_a_batch"):           # at every level: all 70 moves, over a reload
        c = by[name]
        for lvl in c.levels:
            assert [r[0] for r in c.parse("i64", lvl).rows.tolist() if 0 <= r[0] - c.meta["p"] < 200][0] == c.meta["p"] + 70, (name, lvl)
            e = c.model("i64").windows[0][2].schedule(*hm.level_params(lvl))[c.meta["p"] + 70]
            assert e["first_w0"] + e["first"] == c.meta["p"] and e["reloads"] >= 1, (name, lvl, e)
            if name.endswith("batch"): assert e["first_w0"] < 7 * cc.HC_T - 2 <= e["w0"], (lvl, e)      # over the fresh start at 960 j - 2
    assert taken(by["lazy/look_ahead_beyond_last_start/1"], 2)[0] == 0 and taken(by["lazy/look_ahead_beyond_last_start/2"], 2)[0] == 0
    c = by["lazy/look_ahead_beyond_last_start/1"]
    assert c.meta["p"] == len(c.data) - 12
    c = by["lazy/cap_at_p_longer_at_next"]
    assert [tuple(r[:2]) for r in c.parse("i64", 9).rows.tolist() if r[0] >= c.meta["p"]][0] == (c.meta["p"], 270)


def test_back_cases_decide():
    for c in [c for c in cc.corpus() if c.fam == "back"]:
        assert c.attempts == 1
        for fr in c.framings:
            for lvl in c.levels:
                on, off = c.parse(fr, lvl), c.parse(fr, lvl, back=False)
                assert (seqs(on) != seqs(off)) == c.meta["back_differs"], (c.name, fr, lvl)
    by = {c.name: c for c in cc.corpus() if c.fam == "back"}
    pulled = lambda c, fr: [c.meta["p"] - r[0] for r in c.parse(fr, 9).rows.tolist() if r[0] <= c.meta["p"] < r[0] + r[1]][0]
    assert [pulled(by["back/by_%d" % k], "i64") for k in (0, 1, 254, 255, 256)] == [0, 1, 254, 255, 255]
    assert pulled(by["back/clipped_by_the_match_in_front"], "i64") == 10
    assert [pulled(by["back/clipped_by_the_chunk_start"], fr) for fr in ("i256", "l64")] == [5, 5]
    assert pulled(by["back/clipped_by_the_window_start"], "i64") == 3


def test_seam_cases_lie_on_their_seams():
    for c in [c for c in cc.corpus() if c.fam == "seam"]:
        kind, tag = c.name.split("/")[1], c.name.split("/")[2]
        p = c.meta["p"]
        for fr in c.framings:
            P = c.parse(fr, 9)
            rows = P.rows.tolist()
            hit = [r for r in rows if r[0] <= p + c.meta.get("moves", 0) < r[0] + r[1]]
            assert len(hit) == 1, (c.name, fr)
            if kind == "pick": assert hit[0][0] == p and hit[0][1] == (24 if "D" not in c.meta else 40 if c.meta["D"] == 65535 else 8), (c.name, fr, hit)
            if kind == "lazy": assert hit[0][0] == p + 3 and hit[0][1] == 9, (c.name, fr, hit)
            if kind == "reach": assert hit[0][2] == (65535 if c.meta["D"] == 65535 else 3000), (c.name, fr, hit)
            wp = c.meta.get("wp", p)                              # the event's position in its chunk's window
            if "chunk3" in tag: assert wp == p - cc.CHUNK and p >= 2 * cc.CHUNK, c.name
            if tag.startswith("batch") and kind != "reach": assert wp % cc.HC_T == int(tag[5:].split("_")[0]), c.name
            if tag.startswith("lane"):
                # from the parse's schedule (hc_model.Window.schedule: windows of 62 positions from where the last match ended, and a
                # fresh start at every 960 j - 2), at every level: the parse first stands on p in lane R of a window that is 62
                # wide; R = 62, 63 are that window's look-ahead lanes, so the stand is in lane 0, 1 of the next one, loaded at
                # its end; a staircase from lanes 59-61 moves into the look-ahead lanes and is decided again after a reload
                r = int(tag[4:])
                for lvl in c.levels:
                    e = c.model(fr).windows[0][2].schedule(*hm.level_params(lvl))[p + c.meta.get("moves", 0)]
                    assert e["full"] and e["first_w0"] + e["first"] == p, (c.name, lvl, e)
                    assert e["first"] == r % cc.STRIDE and (e["first_w0"] - c.meta["lane0"]) % cc.STRIDE == 0, (c.name, lvl, e)
                    assert e["first_w0"] == c.meta["lane0"] + (cc.LANE_K + r // cc.STRIDE) * cc.STRIDE, (c.name, lvl, e)
                    assert 2 * cc.HC_T - 2 <= c.meta["lane0"] and e["first_w0"] + cc.LANES <= 3 * cc.HC_T - 2, (c.name, e)     # no fresh start between
                    if kind == "lazy": assert (e["reloads"] >= 1) == (r in (59, 60, 61)) and e["w0"] + e["lane"] == p + 3, (c.name, lvl, e)
                    else: assert e["w0"] + e["lane"] == p and e["reloads"] == 0, (c.name, lvl, e)
            if tag.startswith("p"): assert p == int(tag[1:]) and p >= cc.CHUNK
            if tag.startswith("src"): assert p - hit[0][2] == int(tag[3:]), (c.name, fr, hit)
            if tag.startswith("wrap"): assert wp - cc.RING == int(tag[4:].split("_")[0]), c.name
            if kind == "reach":
                assert p % cc.HC_T == (0 if tag == "batch_first" else cc.HC_T - 1) and p > cc.RING, c.name
            if "chunk2" in tag or tag[0] in "psw" or kind == "reach":
                assert p >= cc.CHUNK and fr in ("i256", "l64") and len(c.data) > cc.CHUNK, c.name


def test_raw_cases_lie_on_both_sides():
    for c in [c for c in cc.corpus() if c.fam == "raw"]:
        for fr in c.framings:
            for lvl in c.levels:
                B = c.parse(fr, lvl).blocks
                assert sorted(b["size"] - b["blen"] for b in B) == [-1, 0] and [b["stored"] for b in B] == [b["size"] >= b["blen"] for b in B], (c.name, fr)
    assert {tuple(c.parse("i64", 9).stored) for c in cc.corpus() if c.fam == "raw"} == {(0,), (1,)}


def test_dict_cases_decide():
    for c in [c for c in cc.corpus() if c.fam == "dict"]:
        f = cc.FRAMINGS[c.framings[0]]
        for fr in c.framings:
            f = cc.FRAMINGS[fr]
            for lvl in c.levels:
                P = c.parse(fr, lvl)
                plain = hm.Model(c.data, f["bs"], f["linked"]).parse(lvl, attempts=c.attempts)
                if c.name == "dict/len3":
                    assert not in_dictionary(P) and seqs(P) == seqs(plain), (c.name, fr, lvl)
                else:
                    assert in_dictionary(P) and seqs(P) != seqs(plain), (c.name, fr, lvl)
    by = {c.name: c for c in cc.corpus() if c.fam == "dict"}
    a2, a3 = by["dict/a_passed_over_candidate_costs_an_attempt/A2"], by["dict/a_passed_over_candidate_costs_an_attempt/A3"]
    row = lambda c: [r for r in c.parse("i64", 9).rows.tolist() if r[0] == c.meta["p"]][0]
    assert row(a2)[1] == 10 and row(a3)[1] == 30 and row(a3)[2] == 2000 + 1024 - 100
    c = by["dict/over_the_seam/from_the_dictionary"]
    assert [B["seqs"][-2:] for B in c.parse("i64", 9).blocks][0] == [(1000, 20, 1020), (0, 20, 1020)]      # cut at the seam, and on from the input's first byte
    c = by["dict/back_stops_at_the_seam/input_side"]
    assert (1003, 20, 1003, 1003) in [tuple(r) for r in c.parse("i64", 9).rows.tolist()]
    c = by["dict/back_stops_at_the_seam/dictionary_side"]
    assert (1995, 29, 1995 + 1024, 1995 - 1800) in [tuple(r) for r in c.parse("i64", 9).rows.tolist()], c.parse("i64", 9).rows.tolist()
    assert [row(by["dict/longest_in_the_" + s])[1] for s in ("dictionary", "input")] == [40, 46]
    c = by["dict/second_chunk_does_not_see_it"]
    for fr in c.framings:
        assert all(win.seam == 0 for _, c0, _, _, _, win in c.parse(fr, 9).chunks if c0 > 0)
