"""The case lists of tests/test_gpu_alignment.py (tests/alignment_cases.py) without a GPU: the hand-built frames are what they
are meant to be, the residue pairings cover what they claim, and carve's arithmetic is right.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
import alignment_cases as ac
from conftest import GOLDEN_DIR
from lz4_grammar import corpus

sha = lambda b: hashlib.sha256(b).hexdigest()


def verdict(frame, cap):
    try:
        out, used = oracle.decompress_frame(frame, cap)
        return None, out, used
    except oracle.OracleError as e:
        return str(e), None, None


def test_carve_arithmetic():
    import torch
    for n in (0, 1, 33, 4097, 100000):
        for mis, align in [(m, 64) for m in ac.SRC_RES] + ac.INDEX_RES + [(m, 64) for m in ac.TABLE_RES]:
            for guard in (ac.GUARD, 192):
                v, front, back = ac.carve(n, mis, guard, align=align)
                assert v.dtype == torch.uint8 and v.numel() == n
                base = front.data_ptr()
                at = base + v.storage_offset()                  # (an empty view's data_ptr() is null: go by the offset)
                assert at % align == mis and (n == 0 or v.data_ptr() == at)
                whole = guard + align + n + guard
                # the guards lie inside the allocation, touch the view on both sides, and are at least `guard` bytes each
                assert front.numel() >= guard and back.numel() >= guard
                assert front.numel() == v.storage_offset() and back.storage_offset() == v.storage_offset() + n
                assert back.storage_offset() + back.numel() == whole
                assert front.untyped_storage().nbytes() == whole and front.storage_offset() == 0
                assert ac.intact(front, back) and (n == 0 or bool((v == ac.PAT).all()))
                if n:
                    v.zero_()
                    assert ac.intact(front, back)
                    back[0] = 0
                    assert not ac.intact(front, back)
    with pytest.raises(AssertionError):
        ac.carve(10, 64)


def test_pairings_cover_every_residue():
    for turn in range(6):
        assert sorted(ac.dst_for(f, turn) for f in ac.RES16) == ac.RES16
        assert sorted(ac.frame_for(d, turn) for d in ac.RES16) == ac.RES16
    assert len({tuple(ac.dst_for(f, t) for f in ac.RES16) for t in range(4)}) == 4          # (the turns really differ)
    frames = ac.checksum_frames()
    fres, dres = set(), set()
    for k in range(len(frames)):
        pl = ac.checksum_placements(k)
        assert len(set(pl)) == ac.XXH_RES >= 4 and len({f for f, _ in pl}) == ac.XXH_RES and len({d for _, d in pl}) == ac.XXH_RES
        fres |= {f for f, _ in pl}; dres |= {d for _, d in pl}
    assert fres == dres == set(ac.RES16)


def test_encode_case_list_covers_what_it_claims():
    cases = ac.encode_cases()
    names = set(ac.inputs())
    assert set(ac.SRC_RES) == set(range(16)) | {17, 31, 33, 63} and ac.DST_RES == [0, 1, 3, 8, 13]
    for finder in ac.FINDERS:
        mine = [c for c in cases if c[0] == finder]
        for s in ac.SRC_RES:
            fr = {c[2] for c in mine if c[3] == s and c[1] in ("synth50", "text", "period3")}
            assert fr & set(ac.INDEP) and fr & set(ac.LINKED), (finder, s)
            assert {c[1] for c in mine if c[3] == s} >= {"synth50", "text", "period3"}
        assert {c[2] for c in mine} == set(ac.FRAMINGS)
        assert {c[1] for c in mine} == names
        assert {c[4] for c in mine} == set(ac.DST_RES) and {c[5] for c in mine} == set(ac.TABLE_RES)
        # both loaders' inputs meet every framing
        for name in ("synth50", "text"):
            assert {c[2] for c in mine if c[1] == name} == set(ac.FRAMINGS), (finder, name)
    assert all(c[1] in names and c[2] in ac.FRAMINGS for c in cases)
    assert ac.FINDERS[:2] == ("e1", "e1run") and set(ac.FINDERS) >= {"solo", "hc3", "hc9"}
    assert all(fr in ac.FRAMINGS and s % 4 and 0 <= d < 16 for fr, s, d in ac.BIG_E1) and {fr for fr, _, _ in ac.BIG_E1} == set(ac.FRAMINGS)
    ix = ac.index_cases()
    assert {(c[6], c[5], c[2]) for c in ix} == {(i, t, f) for i in ac.INDEX_RES for t in ac.TABLE_RES for f in ac.FRAMINGS}
    assert {c[0] for c in ix} == set(ac.FINDERS)
    assert all(r % 16 == 0 for r, _ in ac.INDEX_RES) and all(r % 8 == 0 and r % 16 for r in ac.TABLE_RES)
    assert [r for r, _ in ac.INDEX_RES] == [16, 48, 16 + 256]


def test_inputs_are_the_ones_asked_for():
    inp = ac.inputs()
    assert len(inp["synth50"]) == (9 << 20) - 12345 and len(inp["text"]) == (2 << 20) + 777
    assert inp["period3"] == (b"abc" * 100000) and len(inp["period3"]) == 300000
    assert [len(inp["tiny%d" % n]) for n in range(34)] == list(range(34)) and inp["tiny33"] == (b"abcab" * 8)[:33]
    # the oracle's frames of them, in the four framings, decode back (these are the decode sweep's frames)
    for name in ("synth50", "text", "period3", "tiny0", "tiny12", "tiny13", "tiny33"):
        for fr, (bsid, indep, bck, cck) in ac.FRAMINGS.items():
            f = oracle.conduit_compress(inp[name], oracle.mkprefs(bsid=bsid, indep=indep, bck=bck, cck=cck))
            err, out, used = verdict(f, len(inp[name]) + 64)
            assert err is None and out == inp[name] and used == len(f), (name, fr)
            blocks, end = ac.walk(f)
            assert end + (4 if cck else 0) == len(f) and len(blocks) == -(-len(inp[name]) // (1 << (8 + 2 * bsid)))


def test_checksum_frames_and_their_flips():
    frames = ac.checksum_frames()
    seen = set()
    for name, f, content, bck_at, cck_at in frames:
        err, out, used = verdict(f, len(content) + 64)
        assert err is None and out == content and used == len(f), name
        blocks, end = ac.walk(f)
        assert end + 4 == len(f) == cck_at + 4
        assert [p + (w & 0x7FFFFFFF) for p, w in blocks] == bck_at and all(w >> 31 for _, w in blocks), name
        seen |= {w & 0x7FFFFFFF for _, w in blocks}
        assert int.from_bytes(f[cck_at:cck_at + 4], "little") == oracle.xxh32(content)
        for k, at in enumerate(bck_at):
            p, w = blocks[k]
            assert int.from_bytes(f[at:at + 4], "little") == oracle.xxh32(f[p:p + (w & 0x7FFFFFFF)])
            if k in (0, len(bck_at) - 1) or len(f) < (1 << 20):
                err, _, _ = verdict(ac.flip(f, at + k % 4, (k * 5 + 1) % 8), len(content) + 64)
                assert err == "ERROR_blockChecksum_invalid", (name, k, err)
        err, _, _ = verdict(ac.flip(f, cck_at + len(name) % 4, len(f) % 8), len(content) + 64)
        assert err == "ERROR_contentChecksum_invalid", (name, err)
    assert seen >= set(ac.XXH_LENS) - {0} and any(not c for _, _, c, _, _ in frames)         # every length, and the frame of none
    assert ac.XXH_LENS[-2:] == [1 << 20, (4 << 20) - 1]


def test_many_blocks_frame():
    frame, content, blocks = ac.many_blocks_frame()
    assert len(blocks) == ac.MANY_BLOCKS >= 16384 and min(n for _, n in blocks) >= 1 and max(n for _, n in blocks) == 65536
    err, out, used = verdict(frame, len(content) + 64)
    assert err is None and used == len(frame) and sha(out) == sha(content.tobytes())
    wb, end = ac.walk(frame)
    assert end == len(frame) and [(p, w & 0x7FFFFFFF) for p, w in wb] == blocks
    p, n = blocks[len(blocks) // 2]
    bad = frame.copy(); bad[p + n + 1] ^= 0x10
    assert verdict(bad, len(content) + 64)[0] == "ERROR_blockChecksum_invalid"


def test_grammar_subset_is_in_the_golden_file():
    with open(os.path.join(GOLDEN_DIR, "grammar.json")) as f:
        g = json.load(f)["cases"]
    cmap = {n: (f, m) for n, f, m in corpus()}
    assert set(ac.GRAMMAR_SUBSET) == {n.split("/")[0] for n in g} == {"end", "lit", "off", "mext", "lext", "link", "blk", "carrier"}
    for fam, (good, bad) in ac.GRAMMAR_SUBSET.items():
        assert good.startswith(fam + "/") and g[good]["once"]["error"] is None and not good.startswith("off/zero/"), good
        f, m = cmap[good]
        assert sha(f) == g[good]["frame_sha256"] and g[good]["once"]["consumed"] == len(f)
        err, out, used = verdict(f, m["content"])
        assert err is None and sha(out) == g[good]["once"]["out_sha256"] and used == len(f), good
        if bad is None:                                         # the family has no rejected case at all
            assert all(r["once"]["error"] is None for n, r in g.items() if n.startswith(fam + "/")), fam
            continue
        assert bad.startswith(fam + "/") and g[bad]["once"]["error"] is not None, bad
        f, m = cmap[bad]
        assert sha(f) == g[bad]["frame_sha256"]
        for cap in (m["content"], max(len(ac.walk(f)[0]) if fam != "blk" else 2, 1) * m["bs"]):
            err, _, _ = verdict(f, cap)
            assert err is not None and ac.same_verdict(err, g[bad]["once"]["error"]), (bad, cap, err)
    assert not ac.same_verdict("ERROR_blockChecksum_invalid", "ERROR_GENERIC") and ac.same_verdict("ERROR_GENERIC", "ERROR_decompressionFailed")
