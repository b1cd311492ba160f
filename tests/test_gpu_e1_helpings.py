"""Pass E1's long-sequence helpings (k_find_matches, the sparse path) on the smallest inputs that reach them: two to sixteen tiles,
a short last helping and tile, rows that no helping is aligned to, runs of period 1, 4 and 5, a match across a tile boundary behind a
sparse tile, sparse <-> dense between the tiles of one run, and runs that never leave the undecided mode (tests/e1_helping_cases.py).

Every case goes through lz4f_mi355x_dev_compressFrame on an engine whose workgroups take runs of sixteen tiles (so that a run has a
second tile at these sizes) and on one made by default; the frame is decoded by the oracle and by the library, both must return the
input, and its size is held to RATIO_TOL times liblz4's for the same bytes and framing (the oracle's port) - for the inputs that are
one run also to 1 % of the input.

The 70 KiB case is the one that found something: before long helpings were made to end on a multiple of their size (E1_V6 in
encode.cuh) it came out at 1.10-1.13 times liblz4's size in about every second run - the helpings behind a first tile's single
slices began wherever those happened to end, inside a copy row as often as not, and then no copy row with a source less than 10 KiB
back was found.  Four runs of this file since: 1.000-1.014 in every framing on either engine."""
import os

import numpy as np
import pytest

import oracle
import e1_helping_cases as hc
from lz4_frame_conduit_amd import conduit

pytestmark = pytest.mark.gpu

RATIO_TOL = 1.05      # the project's figure: tests/test_gpu_parity.py


def _engine(env):
    from lz4_frame_conduit_amd.device import Engine
    os.environ.update(env)                                                      # (switches are read when an engine is made)
    try:
        return Engine(0)
    finally:
        for k in env: os.environ.pop(k, None)


@pytest.fixture(scope="module")
def engines():
    e = {"run16": _engine(hc.RUN_ENV), "default": _engine({})}
    yield e
    for x in e.values(): x.close()


def _prefs(kw):
    return conduit.make_preferences(blockSizeID=kw["bsid"], blockMode=kw["indep"])


def _compress(eng, data: bytes, kw):
    import torch
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    p = _prefs(kw)
    frame = torch.empty(eng.frame_bound(len(data), p), dtype=torch.uint8, device="cuda")
    eng.compress_async(src, frame, p)                                           # lz4f_mi355x_dev_compressFrame
    r = eng.result()
    return src, frame, int(r.size)


@pytest.mark.parametrize("framing", [f for f, _ in hc.FRAMINGS])
@pytest.mark.parametrize("name", hc.NAMES)
def test_helpings_roundtrip_and_size(engines, name, framing):
    import torch
    data, kw = hc.data(name), dict(hc.FRAMINGS)[framing]
    ref = len(hc.oracle_frame(name, framing))
    for ename, eng in engines.items():
        src, frame, size = _compress(eng, data, kw)
        host = frame[:size].cpu().numpy().tobytes()
        print("%s %s %s: %d bytes, liblz4 %d (x %.4f), %.3f %% of the input" % (name, framing, ename, size, ref, size / ref, 100.0 * size / len(data)))
        out, used = oracle.decompress_frame(host, cap=len(data) + 64)
        assert used == size and out == data, (name, framing, ename, "the oracle's decoder")
        back = torch.zeros_like(src)
        eng.decompress_frame_async(frame, size, back)
        r2 = eng.result()
        assert int(r2.size) == len(data) and torch.equal(back, src), (name, framing, ename, "the library's decoder")
        assert size <= ref * RATIO_TOL, (name, framing, ename, size, ref)
        if name in hc.RUN_CASES:
            assert size * 100 < len(data), (name, framing, ename, size)


def test_deterministic_switch_equal_bytes():
    """LZ4F_MI355X_DETERMINISTIC=1: two fresh engines, equal input, equal bytes."""
    data = hc.data("s50_1m77")
    frames = []
    for _ in range(2):
        eng = _engine({"LZ4F_MI355X_DETERMINISTIC": "1"})
        try:
            _, frame, size = _compress(eng, data, dict(bsid=7, indep=1))
            frames.append(frame[:size].cpu().numpy().tobytes())
        finally:
            eng.close()
    assert frames[0] == frames[1]
    out, used = oracle.decompress_frame(frames[0], cap=len(data) + 64)
    assert used == len(frames[0]) and out == data
