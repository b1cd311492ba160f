"""Pass E1's forward measurement of a match in rows of dwords (E1_V7 in csrc/encode.cuh) on planted inputs: every length at a row's or a
round's edge, every pair of byte phases, distances that overlap the row being compared, a source across the ring's wrap, a match into
a tile's end and into a block's end (tests/e1_match_rows_cases.py; liblz4's side of it in tests/test_e1_match_rows_cpu.py).

Every input goes through lz4f_mi355x_dev_compressFrame on three engines: one made by default, one whose workgroups take runs of sixteen
tiles (only there does a run have a second tile, and its ring a wrap), and the second with one wave parsing, which is a function of its
input.  Every frame is decoded back to the input by the oracle and by the library and keeps the writer rules; the one-wave engine's
parse holds every plant at its planted start, length and distance; the two shared engines' frames stay within RATIO_TOL of liblz4's."""
import os

import numpy as np
import pytest

import oracle
import lz4_writer_rules as wr
import e1_match_rows_cases as mc
from lz4_frame_conduit_amd import conduit

pytestmark = pytest.mark.gpu

RATIO_TOL = 1.05      # the project's figure: tests/test_gpu_parity.py
CASES = [(n, fr) for n in mc.NAMES for fr in mc.CASE_FRAMINGS[n]]


def _engine(env):
    from lz4_frame_conduit_amd.device import Engine
    os.environ.update(env)                                                      # (switches are read when an engine is made)
    try:
        return Engine(0)
    finally:
        for k in env: os.environ.pop(k, None)


@pytest.fixture(scope="module")
def engines():
    e = {"default": _engine({}), "run16": _engine(mc.RUN_ENV), "one_wave": _engine(mc.ONE_WAVE_ENV)}
    yield e
    for x in e.values(): x.close()


def _compress(eng, data: bytes, kw):
    import torch
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    p = conduit.make_preferences(blockSizeID=kw["bsid"], blockMode=kw["indep"])
    frame = torch.empty(eng.frame_bound(len(data), p), dtype=torch.uint8, device="cuda")
    eng.compress_async(src, frame, p)                                           # lz4f_mi355x_dev_compressFrame
    r = eng.result()
    return src, frame, int(r.size)


@pytest.mark.parametrize("ename", ["default", "run16", "one_wave"])
@pytest.mark.parametrize("name,framing", CASES)
def test_planted_matches(engines, name, framing, ename):
    import torch
    eng = engines[ename]
    data, kw = mc.data(name), dict(mc.FRAMINGS)[framing]
    ref = len(mc.oracle_frame(name, framing))
    src, frame, size = _compress(eng, data, kw)
    host = frame[:size].cpu().numpy().tobytes()
    print("%s %s %s: %d bytes, liblz4 %d (x %.4f)" % (name, framing, ename, size, ref, size / ref))
    out, used = oracle.decompress_frame(host, cap=len(data) + 64)
    assert used == size and out == data, "the oracle's decoder"
    back = torch.zeros_like(src)
    eng.decompress_frame_async(frame, size, back)
    r2 = eng.result()
    assert int(r2.size) == len(data) and torch.equal(back, src), "the library's decoder"
    assert wr.audit(host, data, dict(bsid=kw["bsid"], linked=not kw["indep"])) == []
    if ename == "one_wave":
        rows = wr.matches(host).tolist()
        got = {(at, off): ml for at, ml, off, _ in rows}
        want = mc.expected(name, framing)
        missed = [(at, M, D) for at, M, D, _ in want if got.get((at, D)) != M]
        print("%d of %d plants as planted" % (len(want) - len(missed), len(want)))
        # (a plant that is missing, and what the frame has from 64 bytes in front of it to its end instead: start, length, offset, literals)
        assert not missed, [(p, [r for r in rows if p[0] - 64 <= r[0] < p[0] + p[1]]) for p in missed[:6]]
    else:
        assert size <= ref * RATIO_TOL, (size, ref)
