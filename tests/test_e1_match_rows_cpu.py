"""The oracle's side of tests/test_gpu_e1_match_rows.py, and the row form of the forward measurement as a numpy model.

The condition on the inputs (tests/e1_match_rows_cases.py): liblz4's own greedy parse of each takes every plant whole - the matches of
the oracle's frame are the plants, start for start, length for length, distance for distance, cut only five bytes before a block's end.
The model (e1_match_rows_cases.rows_forward: lanes, dword pairs, byte phases, the first row / lane / byte that differs, rounds of 2, 3
and 4 rows) gives what a byte-by-byte comparison gives, for every plant from its first byte and from up to seven bytes into it (a match
is found late as often as not), with and without a limit inside the round."""
import numpy as np
import pytest

import oracle
import lz4_writer_rules as wr
import e1_match_rows_cases as mc

CASES = [(n, fr) for n in mc.NAMES for fr in mc.CASE_FRAMINGS[n]]


@pytest.mark.parametrize("name,framing", CASES)
def test_oracle_takes_every_plant_whole(name, framing):
    d = mc.data(name)
    frame = mc.oracle_frame(name, framing)
    out, used = oracle.decompress_frame(frame, cap=len(d) + 64)
    assert used == len(frame) and out == d
    assert wr.audit(frame, d) == []
    got = [tuple(r) for r in wr.matches(frame).tolist()]
    assert got == [tuple(r) for r in mc.expected(name, framing)]


def test_inputs_cover_what_they_are_for():
    assert all(len(mc.data(n)) == mc.N for n in mc.NAMES)
    m, bl = mc.marks("main"), mc.marks("blocks")
    assert {v[1] for k, v in m.items() if k.startswith("M=")} | {bl["M=4"][1]} == set(mc.LENGTHS) and bl["M=5"][1] == 5
    assert {(v[0] & 3, (v[0] - v[2]) & 3) for k, v in m.items() if k.startswith("phase")} == set(mc.PHASES)
    assert all(v[1] == mc.M_PHASE for k, v in m.items() if k.startswith(("phase", "D=")))
    assert {v[2] for k, v in m.items() if k.startswith("D=")} == {1, 2, 3, 4, 5, 255, 256, 4093, 65535}
    at, M, D = m["source across the wrap"]
    assert mc.TILE <= at < 2 * mc.TILE and at - D < mc.TILE < at - D + M
    at, M, D = m["tile 1 opens inside"]
    assert at < mc.TILE < at + M
    at, M, D = m["into the tile's end"]
    assert at < 2 * mc.TILE < at + M and 2 * mc.TILE - at < 512 and M == 1025
    at, M, D = m["into the block's end"]
    assert at + M == mc.N and 3 * mc.TILE - at > 1536          # (cut by the third tile's end in a later round, by the block's in the first)
    ends = [bl["block %d's end" % k] for k in range(3)]
    assert [at + M for at, M, _ in ends] == [mc.TILE, 2 * mc.TILE, 3 * mc.TILE]
    assert ends[0][1] - 5 < 512 and ends[1][1] - 5 > 1536 and ends[2][1] - 5 in range(764, 769)


@pytest.mark.parametrize("rows", [2, 3, 4])
def test_row_form_is_the_bytewise_count(rows):
    n = 0
    for name in mc.NAMES:
        d = np.frombuffer(mc.data(name), np.uint8)
        rings = {}
        bs = mc.BLOCK[mc.CASE_FRAMINGS[name][0]]
        for at, M, D in mc.case(name).build()[1]:
            tile = at // mc.TILE
            if tile not in rings: rings[tile] = mc.ring_of(d, tile)
            ring = rings[tile]
            te = min((tile + 1) * mc.TILE, len(d))
            bend = min((at // bs + 1) * bs, len(d))
            end_lim = min(te, bend - 5)                                          # where a match may end: the tile's end, five bytes before the block's
            for late in range(0, 8):
                mp = at + late
                if mp + 4 > end_lim or late + 4 > M: break
                for cap in {end_lim - mp, min(end_lim - mp, M - late - 1), min(end_lim - mp, 300)}:
                    want = mc.bytes_forward(ring, mp + mc.TILE, D, cap)
                    assert want == min(M - late, cap)
                    assert mc.rows_forward(ring, mp + mc.TILE, D, cap, rows) == want, (name, at, M, D, late, cap)
                    n += 1
    assert n > 1000
