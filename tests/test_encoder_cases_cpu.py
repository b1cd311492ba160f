"""The encoder edge suite's two helpers, checked without a GPU: lz4_writer_rules.audit tells good frames from bad, and
encoder_cases.corpus is what it says - liblz4's encoder (the oracle) parses every forced case exactly as planted, breaks no writer
rule on any case, and reaches every threshold the corpus names."""

import numpy as np
import pytest

import oracle
import encoder_cases as ec
import lz4_writer_rules as wr
from lz4_grammar import Frame
from lz4_index import Parsed


def oracle_frame(data: bytes, fr: str) -> bytes:
    f = ec.FRAMINGS[fr]
    return oracle.conduit_compress(data, oracle.mkprefs(bsid=f["bsid"], indep=0 if f["linked"] else 1, bck=int(f["bck"]), cck=int(f["cck"])))


@pytest.fixture(scope="module")
def runs():
    """Every case in every framing of its own through the oracle, once: (case, framing) -> (violations, merged matches, shapes, frame
    length, stored flags per block)."""
    out = {}
    for c in ec.corpus():
        data = c.data
        for fr in c.framings:
            frame = oracle_frame(data, fr)
            P = Parsed(frame)
            m = wr.matches(frame, P)
            out[c.name, fr] = (wr.audit(frame, data, ec.FRAMINGS[fr]), m, ec.shapes(P, m), len(frame), [B["stored"] for B in P.blocks])
    return out


def test_liblz4_breaks_no_writer_rule(runs):
    """The reference passes the auditor with no exemption, on every case and framing."""
    bad = {k: v[0] for k, v in runs.items() if v[0]}
    assert not bad, bad


def test_corpus_covers_every_family_and_framing():
    fams = {c.fam for c in ec.corpus()}
    assert fams == {"len", "end", "lit", "mlen", "off", "carry", "raw", "link", "dense"}
    for fr in ec.FRAMINGS:
        assert {c.fam for c in ec.in_framing(fr)} >= {"len", "end", "lit", "mlen"}, fr
    assert all(len(c.data) < (1 << 20) or ec.BS[fr] == ec.B4M for c in ec.corpus() for fr in c.framings)      # big cases: 4 MiB blocks only
    again = {c.name: c for c in ec.cases()}                                        # rebuilt from the names alone
    assert all(again[c.name].data == c.data for c in ec.corpus() if c.forced)


def test_forced_cases_hold_no_repeat_but_the_plants():
    """No 4-byte window occurs twice outside the plants, every plant is a copy that cannot be a byte longer, and no short plant's
    source loses its table slot before the probe."""
    for c in ec.corpus():
        if c.forced:
            data, plants, ghosts = c.build()
            assert len(data) < ec.B4M, c.name
            assert not ec.problems(data, plants, ghosts), (c.name, ec.problems(data, plants, ghosts)[:3])


def test_liblz4_parses_every_forced_case_as_planted(runs):
    """The oracle's parse, neighbours merged, is the planted (position, M, D, L) list - in every framing a case is listed for.  No
    case is left out: the corpus holds only what liblz4 parses as planted."""
    n = 0
    for c in ec.corpus():
        if not c.forced: continue
        for fr in c.framings:
            got = [tuple(r) for r in runs[c.name, fr][1].tolist()]
            assert got == c.expected(ec.BS[fr]), (c.name, fr, got[:4], c.expected(ec.BS[fr])[:4])
            assert runs[c.name, fr][3] == ec.planted_frame_size(c, fr), (c.name, fr)
            n += 1
    assert n > 500


def test_every_threshold_is_some_case(runs):
    """Counted from the oracle's parses: every literal-run, match-length and offset threshold, the writer rules' limits, a stored
    block, a carry across each length-byte threshold and both emit paths occur."""
    seen = set().union(*(v[2] for v in runs.values()))
    assert [s for s in ec.SHAPES if s not in seen] == []


def test_out_of_reach_and_raw_cases_by_size(runs):
    """A repeat 65536 back is no match: the frame is no smaller than the input.  The raw family's payloads are blen - 2, blen - 1
    (compressed) and blen (stored)."""
    by = {c.name: c for c in ec.corpus()}
    for (name, fr), v in runs.items():
        n = len(by[name].data)
        if name in ("off/D65536", "link/reach/D65536", "link/block3_repeats_block1"):
            assert v[3] >= n and all(v[4]), (name, fr)
        if name.startswith("raw/"):
            delta = int(name.rsplit("/", 1)[1])
            blen = n % ec.BS[fr] if n > ec.BS[fr] else n
            overhead = 7 + 4 + 4 * (1 + (n > ec.BS[fr])) * int(ec.FRAMINGS[fr]["bck"]) + 4 * int(ec.FRAMINGS[fr]["cck"]) + (4 + ec.BS[fr] if n > ec.BS[fr] else 0)
            assert v[4][-1] == (delta == 0), (name, fr)
            assert v[3] == overhead + 4 + blen + delta, (name, fr, v[3], overhead, blen)


# ---------------------------------------------------------------------------------------------------------------------
# The auditor on frames made by hand: one broken rule each
def _rng():
    return np.random.default_rng(20240607)


def _good():
    fr = Frame(4, rng=_rng())
    fr.block().s(40, 8, 8).end(12)
    return fr.bytes(), bytes(fr.out), set()


def _match_start():                                         # blen 51: the match starts at 40 = blen - 11
    fr = Frame(4, rng=_rng())
    fr.block().s(40, 6, 8).end(5)
    return fr.bytes(), bytes(fr.out), {"match-start"}


def _match_end():                                           # the match ends at blen - 4: the final run has 4 literals
    fr = Frame(4, rng=_rng())
    fr.block().s(40, 8, 8).end(4)
    return fr.bytes(), bytes(fr.out), {"last-literals"}


def _short_block_match():                                   # a linked frame's second block: 12 bytes, a match at 0 from the block in front
    fr = Frame(4, linked=True, rng=_rng())
    fr.stored(_rng().integers(0, 256, 65536, dtype=np.uint8).tobytes())
    fr.block().s(0, 7, 100).end(5)
    return fr.bytes(), bytes(fr.out), {"short-block-match"}


def _offset_zero():
    fr = Frame(4, rng=_rng())
    fr.block().s(40, 8, 0).end(12)
    return fr.bytes(), bytes(fr.out), {"offset-range"}


def _offset_reach():                                        # position + 1 in an independent block
    fr = Frame(4, rng=_rng())
    fr.block().s(40, 8, 41).end(12)
    return fr.bytes(), bytes(fr.out), {"offset-reach"}


def _far_but_linked():                                      # a linked frame: 65535 back from position 40 is in reach
    fr = Frame(4, linked=True, rng=_rng())
    fr.stored(_rng().integers(0, 256, 65536, dtype=np.uint8).tobytes())
    fr.block().s(40, 8, 65535).end(12)
    return fr.bytes(), bytes(fr.out), set()


def _not_smaller():                                         # 13 literals, a 4-byte match, 8 literals: 25 bytes for 25
    fr = Frame(4, rng=_rng())
    fr.block().s(13, 4, 8).end(8)
    return fr.bytes(), bytes(fr.out), {"not-smaller"}


def _size_word():                                           # a size word above maxBlockSize: then the payload is no smaller either
    fr = Frame(4, rng=_rng())
    fr.block().end(65536)
    return fr.bytes(), bytes(fr.out), {"size-word", "not-smaller"}


def _block_length():                                        # a short block that is not the last
    fr = Frame(4, rng=_rng())
    fr.block().s(40, 8, 8).end(12)
    fr.block().s(40, 8, 8).end(12)
    return fr.bytes(), bytes(fr.out), {"block-length"}


def _stored_too_long():                                     # a stored block of maxBlockSize + 1: its size is its length
    fr = Frame(4, rng=_rng())
    fr.stored(_rng().integers(0, 256, 65537, dtype=np.uint8).tobytes())
    return fr.bytes(), bytes(fr.out), {"size-word", "block-length"}


def _content_length():
    f, d, _ = _good()
    return f, d + b"x", {"content-length"}


def _header_bits():
    fr = Frame(4, bck=True, rng=_rng())
    fr.block().s(40, 8, 8).end(12)
    return fr.bytes(), bytes(fr.out), {"header"}, dict(bsid=4, linked=False, bck=False, cck=False)


def _header_block_size():
    fr = Frame(5, rng=_rng())
    fr.block().s(40, 8, 8).end(12)
    return fr.bytes(), bytes(fr.out), {"header"}, dict(bsid=4)


def _endmark():
    f, d, _ = _good()
    return f[:-4], d, {"endmark"}


def _block_checksum():
    fr = Frame(4, bck=True, rng=_rng())
    fr.block().s(40, 8, 8).end(12)
    f = bytearray(fr.bytes())
    f[-5] ^= 1                                              # (the last byte of the block's checksum, in front of the EndMark)
    return bytes(f), bytes(fr.out), {"block-checksum"}


def _content_checksum():
    fr = Frame(4, cck=True, rng=_rng())
    fr.block().s(40, 8, 8).end(12)
    f = bytearray(fr.bytes())
    f[-1] ^= 1
    return bytes(f), bytes(fr.out), {"content-checksum"}


def _tiny_block_with_match():                               # 4 bytes as literal + match: under 5 bytes the final run must be the whole block
    fr = Frame(4, linked=True, rng=_rng())
    fr.stored(_rng().integers(0, 256, 65536, dtype=np.uint8).tobytes())
    fr.block().s(0, 4, 9).end(0)
    return fr.bytes(), bytes(fr.out), {"last-literals", "short-block-match", "not-smaller"}


HAND = [_good, _far_but_linked, _match_start, _match_end, _short_block_match, _offset_zero, _offset_reach, _not_smaller, _size_word,
        _block_length, _stored_too_long, _content_length, _header_bits, _header_block_size, _endmark, _block_checksum, _content_checksum,
        _tiny_block_with_match]


@pytest.mark.parametrize("make", HAND, ids=[f.__name__[1:] for f in HAND])
def test_auditor_names_the_broken_rule(make):
    """A frame that breaks one rule gets that violation and no other.  (Where one rule cannot be broken alone - a size word above
    maxBlockSize makes the payload no smaller than the block, a match in a block under 5 bytes breaks three - the set says so.)"""
    frame, data, want, *prefs = make()
    assert wr.rules(wr.audit(frame, data, prefs[0] if prefs else None)) == want, wr.audit(frame, data)


def test_every_rule_has_a_hand_made_frame():
    named = set().union(*(make()[2] for make in HAND))
    assert named == {"header", "endmark", "block-checksum", "content-checksum", "size-word", "not-smaller", "block-length", "content-length",
                     "last-literals", "short-block-match", "match-start", "offset-range", "offset-reach"}


def test_hand_made_frames_still_decode():
    """What makes the auditor necessary: liblz4's decoder accepts the frames that break only a writer's rule."""
    for make in (_match_start, _short_block_match, _not_smaller):
        frame, data, *_ = make()
        out, used = oracle.decompress_frame(frame, cap=len(data) + 64)
        assert out == data and used == len(frame), make.__name__
