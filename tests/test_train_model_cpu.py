"""tests/train_model.py - what lz4f_mi355x_dev_trainDict computes - held to its fixture (tests/golden/train_dict_sizes.json, minted with
liblz4 by tools/mint_train_dict_sizes.py), to its own definition word for word, and its small cases (tests/train_cases.py) held to
what their builders planted, so that tests/test_gpu_train_dict.py cannot inherit a wrong expectation.  And the call's C ABI as far as
it goes without a device: declared, exported, bound, refusing a null engine, its constants those of the header."""
import ctypes
import json
import os
import re

import pytest

import train_cases as tc
import train_model as tm
from lz4_frame_conduit_amd import _ffi, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lz4f_mi355x_dev_trainDict"


@pytest.fixture(scope="module", autouse=True)
def the_call_is_declared():
    """the model is the statement of a call: without the call there is nothing these tests hold"""
    assert SYMBOL in _ffi.DECLARED_SYMBOLS, "%s is not bound" % SYMBOL


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "train_dict_sizes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return {c.name: (c, tc.model(c)) for c in tc.all_cases()}


def segments(t: tm.Trained):
    return [x for x in t.log if x[3] not in ("zero", "stale")]


# ---- the fixture ----
def test_corpora_are_the_minted_ones(fx):
    assert fx["defaults"] == tm.DEFAULTS
    for name in tm.CORPORA:
        train, held = tm.records(name)
        assert len(train) == 2048 and len(held) == 256 and {len(x) for x in train + held} == {1024}
        assert tm.sha(b"".join(train)) == fx["corpora"][name]["train_sha256"] and tm.sha(b"".join(held)) == fx["corpora"][name]["held_sha256"]


def test_model_reproduces_the_fixture(fx):
    assert sorted((r["corpus"], r["dict_size"]) for r in fx["rows"]) == sorted((c, s) for c in tm.CORPORA for s in (16384, 65536))
    for r in fx["rows"]:
        t = tm.trained(r["corpus"], r["dict_size"])
        assert tm.sha(t.dict) == r["sha256"], (r["corpus"], r["dict_size"])
        assert (t.used, t.n_segments, t.rounds_run) == (r["used"], r["segments"], r["rounds"])
        C = b"".join(tm.records(r["corpus"])[0])
        check_shape(t, C, r["dict_size"])


def test_trained_beats_naive_beats_none(fx):
    for r in fx["rows"]:
        assert r["trained"] < r["naive"] < r["none"], r


def test_defaults_are_the_grid_best(fx):
    tot = {}
    for g in fx["grid"]:
        tot[(g["k"], g["d"])] = tot.get((g["k"], g["d"]), 0) + g["trained"]
    assert sorted(tot) == sorted((k, d) for k in (64, 128, 256) for d in (6, 8))
    assert min(tot, key=lambda kd: (tot[kd], kd)) == (tm.DEFAULTS["k"], tm.DEFAULTS["d"])
    for r in fx["rows"]:                                                      # (the grid's default cell is the 64 KiB row)
        if r["dict_size"] == 65536:
            assert [g["trained"] for g in fx["grid"] if (g["corpus"], g["k"], g["d"]) == (r["corpus"], tm.DEFAULTS["k"], tm.DEFAULTS["d"])] == [r["trained"]]


# ---- the shape of every output ----
def check_shape(t: tm.Trained, C: bytes, dict_size: int):
    assert len(t.dict) == dict_size and 0 <= t.used <= dict_size and t.consumed == len(C)
    assert t.dict[:dict_size - t.used] == bytes(dict_size - t.used)
    segs = segments(t)
    assert t.n_segments == len(segs) and sum(s[3][2] for s in segs) == t.used
    at = dict_size
    for _, _, _, (s0, s1, take) in segs:                                      # every segment a substring of C, laid down from the end
        at -= take
        assert take >= 1 and t.dict[at:at + take] == C[s0:s0 + take]
    assert 1 <= t.rounds_run <= 64 or (t.rounds_run == 0 and t.used == 0)


def test_every_case_is_consistent(cases):
    for name, (c, t) in cases.items():
        C, bad = tm.corpus(c.src, c.off, c.src_bytes)
        check_shape(t, C, c.dict_size)
        assert t.first_bad == bad and t.rounds_run <= c.params["rounds"], name
        assert tc.model(c) == t, name                                         # a second run: the same bytes, the same log
        if c.naive:
            assert tm.train_naive(C, c.dict_size, c.params, bad) == t, name


def test_cases_show_what_they_were_built_for(cases):
    t = cases["n/below_d"][1]
    assert (t.used, t.rounds_run, t.consumed, t.dict) == (0, 0, 3, bytes(64))
    t = cases["n/equals_d"][1]
    assert t.used == 4 and t.dict[-4:] == b"abcd"
    for n in (15, 16, 17):
        c, t = cases["n/k%+d" % (n - 16)]
        assert tm._shape(n, 64, 16, 4)[2] == (1 if n <= 16 else 2)
    c, t = cases["small_corpus"]
    assert t.used < c.dict_size and [x for x in t.log if x[0] == t.rounds_run - 1 and x[3] not in ("zero", "stale")] == []      # ended on "nothing appended"
    for ds in (1, 15, 16, 17, 53):
        t = cases["dict_size/%d" % ds][1]
        assert t.used == ds                                                   # full: the last segment cut to the room that was left
    assert segments(cases["dict_size/53"][1])[-1][3][2] < 16
    assert cases["rounds/1"][1].rounds_run == 1 and cases["rounds/1"][1].used < 300
    assert cases["rounds/2"][1].rounds_run == 2
    t = cases["same_sample_x64"][1]
    first = [x for x in t.log if x[0] == 0]
    assert len(first) == 64 and len({x[2] % 256 for x in first}) == 1 and [x[3] == "stale" for x in first] == [False] + [True] * 63
    t = cases["one_byte_4k"][1]
    assert (t.n_segments, t.used, t.rounds_run) == (1, 16, 2)                 # one distinct hash: the first window takes it, the next round finds nothing
    c, t = cases["tie/one_epoch"]
    assert t.log[0][2] < 9 + 40                                               # the first of the two equal windows
    assert "tie/epoch_last_start" in cases and "tie/across_seam" in cases
    t = cases["tie/across_seam"][1]
    assert [x[3] == "stale" for x in t.log if x[0] == 0] == [False, True]
    t = cases["stale/planted"][1]
    assert [x[3] == "stale" for x in t.log if x[0] == 0] == [False, True]
    assert [x for x in t.log if x[0] == 1 and x[1] == 1][0][3] not in ("zero", "stale")
    c, t = cases["spans/reversed_and_past"]
    assert t.first_bad == 1 and t.consumed == 500
    assert cases["spans/overlap"][1].first_bad == 1 and cases["spans/overlap"][1].consumed == 300 + 300 + 0
    assert cases["spans/descending"][1].first_bad == 1 and cases["spans/descending"][1].consumed == 600
    assert cases["spans/overrun"][1].consumed == 600 and cases["spans/overrun"][1].first_bad == 1
    assert cases["empty_between"][1].consumed == 600


def test_epoch_formula_of_the_kernels():
    """k_td_pick finds a start's epoch by ((p + 1) * E - 1) / W: the largest e with e * W / E <= p"""
    for W in (1, 2, 3, 7, 10, 64, 100, 4097):
        for E in {1, 2, 3, W // 2 or 1, W - 1 or 1, W}:
            if E > W: continue
            want = [e for e in range(E) for _ in range(e * W // E, (e + 1) * W // E)]
            assert [((p + 1) * E - 1) // W for p in range(W)] == want, (W, E)


# ---- the ABI ----
def test_symbol_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()
    assert re.search(r"LZ4F_MI355X_API\s+size_t\s+%s\s*\(" % SYMBOL, hdr)
    assert SYMBOL in _ffi.DECLARED_SYMBOLS
    assert ctypes.sizeof(_ffi.TrainParams) == 32
    num = lambda name: int(re.search(r"#define\s+%s\s+(\d+)u" % name, hdr).group(1))
    assert (num("LZ4F_MI355X_TRAIN_TILE"), num("LZ4F_MI355X_TRAIN_SCAN_TILE")) == (device.TRAIN_TILE, device.TRAIN_SCAN_TILE) == (tc.TILE, tc.SCAN_TILE)
    got = {"k": num("LZ4F_MI355X_TRAIN_K"), "d": num("LZ4F_MI355X_TRAIN_D"), "f": num("LZ4F_MI355X_TRAIN_F"), "rounds": num("LZ4F_MI355X_TRAIN_ROUNDS")}
    assert got == device.TRAIN_DEFAULTS == tm.DEFAULTS


def test_null_engine_is_refused():
    L = _ffi.lib()
    f = getattr(L, SYMBOL)
    assert len(f.argtypes) == 9
    assert L.LZ4F_isError(f(None, 1, None, 0, None, None, 0, None, None))
