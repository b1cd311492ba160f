"""The oracle against liblz4 1.9.3 on the LZ4 block grammar's edges (tests/lz4_grammar.py; the verdicts in
tests/golden/grammar.json were recorded from liblz4 by oracle/mint_golden.py).  CPU only."""
import hashlib
import json
import os

import pytest

import oracle
from conftest import GOLDEN_DIR, golden_file
from lz4_grammar import corpus

sha = lambda b: hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def grammar():
    with open(os.path.join(GOLDEN_DIR, "grammar.json")) as f:
        return json.load(f)


# liblz4 1.9.3 names a block that does not decode ERROR_GENERIC when it decodes straight into the caller's buffer (a block's room
# left there) and ERROR_decompressionFailed when it decodes into its own block buffer (less left); the recorded verdicts are
# for room = the content size, where the oracle must give the same name
BLOCK_FAILED = ("ERROR_GENERIC", "ERROR_decompressionFailed")


def oracle_verdict(frame: bytes, cap: int):
    try:
        out, used = oracle.decompress_frame(frame, cap)
        return None, sha(out), used
    except oracle.OracleError as e:
        return str(e), None, None


def test_corpus_is_the_recorded_one(grammar):
    cases = corpus()
    assert sorted(n for n, _, _ in cases) == sorted(grammar["cases"])
    for name, frame, meta in cases:
        g = grammar["cases"][name]
        assert (sha(frame), meta["content"]) == (g["frame_sha256"], g["content"]), name


def test_oracle_gives_liblz4s_verdicts(grammar):
    """Every case, with room = the content size and with a block's room more: liblz4's error name, or its bytes and the
    bytes consumed.  liblz4 judges a block against maxBlockSize whatever the capacity (LZ4F_decompress decodes into tmpOut
    when the caller's buffer is smaller), so the verdict must not depend on the capacity.  The one recorded deviation:
    offset 0, which liblz4 1.9.3 accepts (the match copies bytes nobody wrote) and the oracle, like every decoder of this
    library, rejects."""
    accepted = rejected = 0
    for name, frame, meta in corpus():
        g = grammar["cases"][name]
        once, pieces = g["once"], g["pieces"]
        # liblz4 itself: one call and small pieces agree (but for what offset 0 reads, which is whatever the buffer held)
        assert (once["error"] is None) == (pieces["error"] is None), name
        zero = name.startswith("off/zero/")
        if not zero:
            assert once["out_sha256"] == pieces["out_sha256"], name
            assert once["error"] == pieces["error"] or {once["error"], pieces["error"]} <= set(BLOCK_FAILED), name
        for cap in (meta["content"], meta["content"] + 5, meta["content"] + meta["bs"]):
            err, osha, used = oracle_verdict(frame, cap)
            if zero:
                assert once["error"] is None and err in BLOCK_FAILED, (name, cap, err)
            elif once["error"] is None:
                assert err is None and osha == once["out_sha256"] and used == once["consumed"], (name, cap, err)
            elif cap == meta["content"] or once["error"] not in BLOCK_FAILED:
                assert err == once["error"], (name, cap, err, once["error"])
            else:                                                       # (the name of a failed block depends on the room: below)
                assert err in BLOCK_FAILED, (name, cap, err, once["error"])
        if once["error"] is None and meta["content"] > 0 and not zero:
            err, _, _ = oracle_verdict(frame, meta["content"] - 1)            # one byte short: the one-shot call says so
            assert err == "ERROR_dstMaxSize_tooSmall", (name, err)
        accepted += once["error"] is None
        rejected += once["error"] is not None
    assert accepted > 200 and rejected > 100, (accepted, rejected)


def test_boundary_pairs_are_pairs(grammar):
    """The corpus does what it is for: each boundary has its last accepted and its first rejected shape."""
    v = {n: c["once"]["error"] for n, c in grammar["cases"].items()}
    for kind in ("sparse", "dense"):
        for bs in ("", "bsid5/", "bsid7/"):
            full, short = "end/%s/full/%s" % (kind, bs), "end/%s/short/%s" % (kind, bs)
            if not (kind == "dense" and bs == "bsid7/"):                                    # (not made: see lz4_grammar)
                assert v[full + "M8/k5"] is None and v[full + "M8/k4"] is not None, bs      # the last match ends room - 5 / room - 4
                assert v[full + "M4/k8"] is None and v[full + "M4/k7"] is not None, bs      # ... and starts room - 12 / room - 11
            assert v[short + "M4/k5"] is None and v[short + "M4/k4"] is not None, bs        # final literals: iend - ip >= 8 behind a run
            assert v[short + "M8/k5"] is None and v[short + "M4/k0"] is not None, bs        # (room is maxBlockSize, not the block's end)
        assert v["end/%s/short/M281/k4" % kind] is None and v["end/%s/short/M281/k3" % kind] is not None    # two length bytes count
        assert v["end/%s/full_d-1/M8/k5" % kind] is None and v["end/%s/full_d+1/M8/k5" % kind] is not None   # decodes to bs / bs + 1
    for L in (40, 300):
        assert v["end/lit12/L%d/+0" % L] is None and v["end/lit12/L%d/+1" % L] is not None
    for where in ("first", "mid"):
        assert v["off/reach/%s/L4/+0" % where] is None and v["off/reach/%s/L4/+1" % where] is not None
    for bsid in (4, 7):
        for h in ("none", "100+200", "10+20+30+40", "stored500"):
            assert v["link/bsid%d/hist_%s/+0" % (bsid, h)] is None and v["link/bsid%d/hist_%s/+1" % (bsid, h)] is not None, (bsid, h)
    for bsid in (4, 5):
        assert v["blk/payload_bs/bsid%d/+0" % bsid] is None and v["blk/payload_bs/bsid%d/+1" % bsid] == "ERROR_maxBlockSize_invalid"
        assert v["blk/stored_bs/bsid%d/+0" % bsid] is None and v["blk/stored_bs/bsid%d/+1" % bsid] == "ERROR_maxBlockSize_invalid"


def test_hc_frames(grammar):
    """liblz4's HC frames (levels 9 and 12) of the project's own sources: the oracle gives the text back."""
    import lzma
    text = lzma.decompress(golden_file("project_sources.txt.xz"))
    for name, g in grammar["hc"].items():
        fr = golden_file(g["file"])
        assert sha(fr) == g["frame_sha256"] and sha(text) == g["input_sha256"], name
        for cap in (len(text), len(text) + 5, len(text) + (1 << 18)):
            out, used = oracle.decompress_frame(fr, cap)
            assert out == text and used == len(fr), (name, cap)
