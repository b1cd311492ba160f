"""The tile merge's model and cases (tests/e1_merge_cases.py), checked for self-consistency on the CPU: the kept records tile, the
literal runs add up, and the cases are the shapes they are meant to be."""
import numpy as np
import pytest

import e1_merge_cases as mc


@pytest.fixture(scope="module")
def tiles():
    return mc.cases()


def test_kept_records_tile_and_literals_add_up(tiles):
    for t in tiles:
        m = mc.model(t, "found")
        assert m["room"] or t.name == "pool_short1", t.name
        full = mc.model(mc_roomy(t), "kept")
        recs = mc.unpack(full["recs"], t.ts)
        pos, body = t.ts, 0
        for st, ml, off in recs:
            assert st >= pos and ml >= mc.MINMATCH and 1 <= off <= 65535, (t.name, st, pos, ml)
            assert st + ml <= t.end_lim and (st + mc.MFLIMIT <= t.bend), (t.name, st, ml)      # where a match may start and end
            body += mc.seq_size(st - pos, ml)
            pos = st + ml
        assert full["nrec"] == len(recs) and full["body_size"] == body, t.name
        assert sum((int(x) & 0xFFFFFF) + ((int(x) >> 24) & 0xFFFFFF) for x in full["recs"]) + full["tail_lit"] == t.te - t.ts, t.name
        assert full["first_lit"] == (recs[0][0] - t.ts if recs else 0) and full["tail_lit"] == t.te - pos, t.name
        assert full["nrec"] <= full["found"], t.name


def mc_roomy(t):
    """the same tile with a pool nothing can exhaust"""
    import copy
    r = copy.copy(t)
    r.pool = 1 << 20
    return r


def test_the_two_reservation_rules_agree_on_every_case(tiles):
    """kept (before round 7) and found (E1_V9) differ in the pool's bump pointer and nowhere else, on these tiles"""
    for t in tiles:
        a, b = mc.model(t, "kept"), mc.model(t, "found")
        for k in ("nrec", "first_lit", "tail_lit", "body_size", "mode", "room", "noroom"):
            assert a[k] == b[k], (t.name, k)
        assert np.array_equal(a["recs"], b["recs"]) and a["bump"] <= b["bump"], t.name


def test_cases_are_what_they_say(tiles):
    by = {t.name: t for t in tiles}
    m = {n: mc.model(by[n], "found") for n in by}
    assert m["empty"]["nrec"] == 0 and m["empty"]["tail_lit"] == mc.E1_TILE and m["empty"]["bump"] == 0 and m["empty"]["mode"] == 1
    assert m["bench"]["nrec"] == m["bench"]["found"] == 64 and int(by["bench"].s_n.max()) == 1
    assert int(by["lists_le2"].s_n.max()) == 2 and int(by["lists_3"].s_n.max()) == 3 and int((by["lists_3"].s_n == 3).sum()) <= 5
    assert set(np.unique(by["lists_mixed"].s_n)) == {0, 1, 2, 3, 4, 32} and m["lists_mixed"]["mode"] == 2
    assert by["lists_one_long"].s_n[-1] == 32 and int(by["lists_one_long"].s_n[:-1].max()) == 2
    for name, k in (("cover_1", 1), ("cover_7", 7), ("cover_8", 8), ("cover_9", 9), ("cover_64", 64), ("cover_300", 300)):
        t = by[name]
        recs = mc.unpack(m[name]["recs"], t.ts)
        big = [r for r in recs if r[2] == 4000]
        assert len(big) == 1 and big[0][1] > k * mc.E1_SLICE, name
        under = [r for r in recs if big[0][0] < r[0] < big[0][0] + big[0][1]]
        assert not under and m[name]["nrec"] < m[name]["found"] - 2 * (k - 1), name      # the lists under it are gone
    keep4, drop3 = mc.unpack(m["straddle_keep4"]["recs"], by["straddle_keep4"].ts), mc.unpack(m["straddle_drop3"]["recs"], by["straddle_drop3"].ts)
    assert [r[1] for r in keep4 if r[2] == 200] == [mc.MINMATCH] and not [r for r in drop3 if r[2] == 200]
    assert m["straddle_keep4"]["nrec"] == 3 and m["straddle_drop3"]["nrec"] == 2
    assert m["straddle_keep5"]["nrec"] == 2 and m["straddle_mflimit"]["nrec"] == 1      # the same five bytes: the block's end decides
    for ns in (1, 7, 8, 9, 511):
        t = by["nslice_%d" % ns]
        assert t.nslice == ns and int(t.s_n[ns:].min()) >= 1 and m[t.name]["found"] == int(t.s_n[:ns].sum()) and m[t.name]["nrec"] >= 1
    assert m["first_in_lane5"]["first_lit"] == 43 * mc.E1_SLICE + 5 and m["last_slice_only"]["nrec"] == 1
    assert m["pool_exact"]["room"] and m["pool_exact"]["nrec"] == 64 and m["pool_exact"]["base"] == 1000
    assert not m["pool_short1"]["room"] and m["pool_short1"]["nrec"] == 0 and m["pool_short1"]["tail_lit"] == mc.E1_TILE and m["pool_short1"]["noroom"] == 1
    rnd = [n for n in by if n.startswith("random")]
    assert len(rnd) == 200
    assert sum(1 for n in rnd if m[n]["nrec"] < m[n]["found"]) > 50              # tiles that drop records
    assert sum(1 for n in rnd if int(by[n].s_n.max()) <= 2) > 5 and sum(1 for n in rnd if int(by[n].s_n.max()) > 32) > 5
    assert sum(1 for n in rnd if by[n].nslice < mc.E1_NSLICE) > 20 and sum(1 for n in rnd if m[n]["mode"] == 2) > 10
