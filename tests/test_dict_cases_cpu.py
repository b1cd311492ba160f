"""The shared-dictionary fixture (tests/golden/dict_frames.json, minted from liblz4 by tools/mint_dict_golden.py) against the
dictionary model of dict_cases.py: the model must give liblz4's verdict and liblz4's bytes on every frame - it is what the GPU
tests hold the device to - and the fixture must be the one these generators were minted with."""
import base64

import pytest

import dict_cases as dc


@pytest.fixture(scope="module")
def fx():
    return dc.load_fixture()


def test_fixture_is_the_minted_one(fx):
    dc.check_sha(fx)
    assert set(fx["dicts"]) == set(dc.DICT_LEN)
    for dname in dc.DICT_LEN:
        for mode in dc.MODES:
            names = {e["name"] for e in fx["natural"] if e["dict"] == dname and e["mode"] == mode}
            want = {n for n, data in dc.natural(dname) if mode == "indep" or len(data) > dc.KB64}      # (a single block is never linked)
            assert names == want, (dname, mode)


@pytest.mark.parametrize("dname", list(dc.DICT_LEN))
def test_model_decodes_liblz4_frames(fx, dname):
    d = dc.dictionary(dname)
    n = 0
    for e in fx["natural"]:
        if e["dict"] != dname: continue
        frame, data = base64.b64decode(e["frame"]), dict(dc.natural(dname))[e["name"]]
        v = dc.model_decode(frame, d)
        assert v.ok and v.out == data and v.consumed == len(frame), (dname, e["mode"], e["name"], v.why)
        assert dc.walk(frame)["linked"] == (e["mode"] == "linked")
        n += 1
    assert n >= 8


@pytest.mark.parametrize("dname", list(dc.DICT_LEN))
def test_model_agrees_with_liblz4_on_planted_frames(fx, dname):
    d = dc.dictionary(dname)
    frames = {(m, n): f for n, m, f in dc.planted(dname)}
    seen = {"ok": 0, "bad": 0}
    for e in fx["planted"]:
        if e["dict"] != dname: continue
        v = dc.model_decode(frames[(e["mode"], e["name"])], d)
        assert v.ok == e["ok"], (dname, e["mode"], e["name"], v.why)
        if e["ok"]:
            assert len(v.out) == e["out_len"] and dc.sha(v.out) == e["out_sha256"], (dname, e["mode"], e["name"])
            seen["ok"] += 1
        else:
            assert v.bad_block == e["bad_block"], (dname, e["mode"], e["name"], v.bad_block, e["bad_block"])
            seen["bad"] += 1
    assert seen["ok"] >= 10
    assert seen["bad"] >= 3 or dc.DICT_LEN[dname] + 11 > 65535      # (no offset reaches in front of a dictionary of 64 KiB)


def test_planted_frames_reach_into_the_dictionary(fx):
    """What the planted frames are for: without the dictionary the model rejects them (all but the far third block, whose
    offset lands in the frame's own output)."""
    for dname in dc.DICT_LEN:
        for name, mode, frame in dc.planted(dname):
            v = dc.model_decode(frame, b"")
            assert v.ok == (name == "third_block_far"), (dname, mode, name)


def test_liblz4_gains_threefold_on_the_small_records(fx):
    """The ratio test of the GPU suite has teeth only if the dictionary matters to liblz4 itself: over the phrase dictionary's
    records of at most 4096 bytes its frames are at least 3x smaller with the dictionary than without."""
    t = fx["totals"]["phrase"]
    assert t["records"] >= 40 and t["without"] >= 3 * t["with"], t
    small = [e for e in fx["natural"] if e["dict"] == "phrase" and e["len"] <= dc.RATIO_MAX]
    assert sum(len(base64.b64decode(e["frame"])) for e in small) == t["with"] and len(small) == t["records"]
