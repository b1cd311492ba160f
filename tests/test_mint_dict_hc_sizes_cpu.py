"""tests/golden/dict_hc_sizes.json (tools/mint_dict_hc_sizes.py): liblz4's totals for the ratio corpus with a dictionary, level by
level.  The fixture is the one minted from the dictionary and the inputs that tests/dict_cases.py regenerates, and its numbers say what
they are there to say: a dictionary helps at every level, and the chain search helps on top of it.  liblz4 is not needed."""
import json
import os

import pytest

import dict_cases as dc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict_hc_sizes.json")
LEVELS = (0, 3, 6, 9, 12)


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE) as f:
        return json.load(f)


def test_hashes_are_the_regenerated_corpus(fx):
    d = dc.dictionary(fx["dict"]["name"])
    assert fx["dict"]["name"] == "phrase" and fx["dict"]["len"] == len(d) and fx["dict"]["sha256"] == dc.sha(d)
    corpus = [(name, data) for name, data in dc.natural("phrase") if len(data) <= dc.RATIO_MAX]
    assert [(e["name"], e["len"], e["sha256"]) for e in fx["inputs"]] == [(name, len(data), dc.sha(data)) for name, data in corpus]
    assert fx["records"] == len(corpus) == 49
    assert fx["bytes"] == sum(len(data) for _, data in corpus) == 32729


def test_sizes_and_hashes_only(fx):
    assert set(fx) == {"liblz4", "dict", "inputs", "records", "bytes", "totals"}
    assert set(fx["totals"]) == {str(level) for level in LEVELS}
    for t in fx["totals"].values():
        assert set(t) == {"with", "without"} and all(isinstance(v, int) and v > 0 for v in t.values())
    assert os.path.getsize(FIXTURE) < 16384


def test_a_dictionary_helps_and_the_chain_search_helps_more(fx):
    t = fx["totals"]
    for level in LEVELS:
        assert t[str(level)]["with"] < t[str(level)]["without"], level
    for level in LEVELS[1:]:
        assert t[str(level)]["with"] <= t["0"]["with"], level
