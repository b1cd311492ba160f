"""lz4f_mi355x_dev_splitFrames (Engine.split_frames_async): the frame boundaries of a concatenated LZ4 stream, found on the device.

Every case runs through an engine as made (the parallel kernels: candidates, extents, links, reachability) and through an engine made
with LZ4F_MI355X_SPLIT_SERIAL (one thread walks), and is held to tests/split_model.py - itself held to the oracle and to what its case
builders planted by tests/test_split_model_cpu.py - for the offsets and every field of the record but the path bits, which the case
asserts itself: both paths are shown to run.  Offsets and record carry guards that must survive.  The chains end in the batch
decoder: the split's offsets are what measure_frames_async and decompress_frames_async take as they are."""
import os

import numpy as np
import pytest
import torch

import dict_cases as dc
import oracle
import split_model as sm
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_frame_conduit_amd._ffi import Result
from lz4_frame_conduit_amd.device import Engine, frame_windows, pack_directory_size

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT = 0xA5
OFF_PAT = -0x5A5A5A5A5A5A5A5B
SERIAL, PARALLEL = sm.PATH_BATCH, sm.PATH_BATCH | sm.PATH_PARALLEL_WALK


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ser():
    """an engine that skips the parallel kernels (the switch is read when the engine is made)"""
    os.environ["LZ4F_MI355X_SPLIT_SERIAL"] = "1"
    try:
        e = Engine(0)
    finally:
        del os.environ["LZ4F_MI355X_SPLIT_SERIAL"]
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sm.all_cases()}


def shifted(data: bytes, shift: int = 0) -> torch.Tensor:
    """data in device memory, `shift` bytes past an allocation's (256-byte aligned) start"""
    t = torch.full((shift + len(data) + 1,), PAT, dtype=torch.uint8, device=DEV)
    if data:
        t[shift:shift + len(data)].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    return t[shift:shift + len(data)]


def run_split(e, stream: bytes, max_frames: int, shift: int = 0, want_record: bool = True):
    """One call held to the model, guards and all -> (the record's path bits, the offsets' tensor, the stream's tensor)"""
    want_off, want_rec = sm.split(stream, max_frames)
    src = shifted(stream, shift)
    off_all = torch.full((4 + max_frames + 1 + 4,), OFF_PAT, dtype=torch.int64, device=DEV)
    rec_all = torch.full((96,), PAT, dtype=torch.uint8, device=DEV)
    off = off_all[4:4 + max_frames + 1]
    if stream:
        e.split_frames_async(src, max_frames, off, record=rec_all[32:64] if want_record else None)
    else:                                                                      # (an empty tensor has no address: the C ABI, with one)
        spot = torch.zeros(1, dtype=torch.uint8, device=DEV)
        assert e.L.lz4f_mi355x_dev_splitFrames(e.h, spot.data_ptr(), 0, max_frames, off.data_ptr(), rec_all[32:64].data_ptr() if want_record else None) == 0
    e.stream.synchronize()
    got_off, got_rec = off_all.cpu().numpy(), rec_all.cpu().numpy()
    assert (got_off[:4] == OFF_PAT).all() and (got_off[4 + max_frames + 1:] == OFF_PAT).all(), "offsets outside the max_frames + 1 were written"
    assert (got_rec[:32] == PAT).all() and (got_rec[64:] == PAT).all(), "bytes around the record were written"
    assert got_off[4:4 + max_frames + 1].tolist() == want_off
    if not want_record:
        assert (got_rec == PAT).all()
        return None, off, src
    r = Result.from_buffer_copy(got_rec[32:64].tobytes())
    got = sm.Rec(r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags & 0xFFF)
    assert got == want_rec, (got, want_rec)
    return r.flags >> 12, off, src


def both(eng, ser, stream: bytes, max_frames: int, shift: int = 0, overflows: bool = False):
    """The call on both engines; each says which kernels delivered"""
    assert run_split(ser, stream, max_frames, shift)[0] == SERIAL
    path, off, src = run_split(eng, stream, max_frames, shift)
    assert path == (SERIAL if overflows else PARALLEL), hex(path)
    return off, src


def run_case(eng, ser, c):
    n = len(c.planted.starts)
    return both(eng, ser, c.stream, max(n, 1) if c.max_frames is None else c.max_frames, overflows=c.serial)      # (max_frames 0 enqueues nothing)


# ---- the grammar's edges ----
def test_grammar_edges(eng, ser, cases):
    """Headers of 7, 11, 15 and 19 bytes, block and content checksums, stored and empty stored blocks, linked and independent frames,
    all four block sizes, the oracle's frames, runs of 11- and of 15-byte frames"""
    c = cases["grammar"]
    assert len(c.planted.starts) > 160 and c.planted.status == 0
    run_case(eng, ser, c)


def test_one_frame_of_5000_blocks(eng, ser, cases):
    run_case(eng, ser, cases["depth/5000_blocks"])


# ---- positions ----
@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_every_alignment_gives_the_same_answer(eng, ser, cases, shift):
    c = cases["short"]
    both(eng, ser, c.stream, len(c.planted.starts), shift=shift)
    both(eng, ser, cases["pos/unit"].stream, len(cases["pos/unit"].planted.starts), shift=shift)


def test_magic_and_header_across_unit_and_chunk_boundaries(eng, ser, cases):
    names = [n for n in cases if n.startswith("pos/")]
    assert len(names) == 9
    for n in names:
        run_case(eng, ser, cases[n])
    run_split(eng, cases["pos/unit"].stream, 5, want_record=False)            # the record is optional
    run_split(ser, cases["pos/unit"].stream, 5, want_record=False)


def test_stream_ends(eng, ser, cases):
    """A frame that ends exactly at srcBytes (every case that ends well), 1..3 bytes before it, and no stream at all"""
    for n in (1, 2, 3):
        c = cases["stop/%d_bytes_behind" % n]
        assert c.planted.status == sm.ST_INCOMPLETE and c.planted.pos == len(c.stream) - n
        run_case(eng, ser, c)
    both(eng, ser, b"", 3)


# ---- depth ----
@pytest.mark.parametrize("n", [2051, 66000])
def test_scan_and_doubling_depth(eng, ser, cases, n):
    c = cases["depth/%d" % n]
    assert len(c.planted.starts) == n
    off, _ = run_case(eng, ser, c)
    assert off[-1].item() == 11 * n


# ---- skippable frames ----
def test_skippable_frames(eng, ser, cases):
    """Each of the 16 magics between frames, size 0, at the end; this library's trailer behind a frame; a skippable frame that holds a
    whole valid frame"""
    for n in ("skip/magics", "skip/trailer", "skip/holds_a_frame"):
        assert cases[n].planted.skipped
        run_case(eng, ser, cases[n])


# ---- false candidates ----
def test_false_candidates_are_not_reachable(eng, ser, cases):
    """A whole valid frame inside a stored block (at payload offsets 0 and 1 and at its end), one that the outer frame's EndMark closes
    so that it ends exactly on the next true frame's start, a frame nested three deep, lone and broken magics inside payloads: the
    parallel kernels deliver all the same"""
    for n in ("false/whole_frame", "false/closed_by_outer_endmark", "false/nested", "false/magics"):
        assert sm.nodes(cases[n].stream) > len(cases[n].planted.starts)         # (the root is the first frame)
        run_case(eng, ser, cases[n])


# ---- stops ----
def test_stops(eng, ser, cases):
    """The frames before the stop are listed, the stopping frame is not"""
    names = [n for n in cases if n.startswith("stop/")]
    assert len(names) >= 14
    for n in names:
        c = cases[n]
        assert c.planted.status != 0
        off, _ = run_case(eng, ser, c)
        assert off[-1].item() == c.planted.pos


def test_last_frame_truncated_at_every_byte(eng, ser):
    stream, a = sm.truncation_stream()
    for cut in range(a, len(stream) + 1):
        both(eng, ser, stream[:cut], 2)


# ---- max_frames ----
def test_max_frames(eng, ser, cases):
    for name, m in (("n", 6), ("n-1", 5), ("1", 1), ("4n", 24)):
        c = cases["max_frames/" + name]
        assert c.max_frames == m and len(c.planted.starts) == 6
        off, src = run_case(eng, ser, c)
        got = off.cpu().tolist()
        if m < 6:
            assert got[m] == c.planted.starts[m]                              # the span of the last frame listed ends where the next frame starts
        else:
            assert got[6:] == [c.planted.pos] * (m - 5)
    # the surplus slots are empty spans: the batch decoder gives them frameHeader_incomplete, and decodes the others
    n, m = 6, 24
    res, dst_off = eng.new_results(m), torch.zeros(m + 1, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(src, off, res, dst_off)
    dst = torch.full((4096,), PAT, dtype=torch.uint8, device=DEV)
    eng.decompress_frames_async(src, off, dst, dst_off, res)
    recs = eng.frame_results(res)
    assert [r.status for r in recs] == [0] * n + [sm.ST_INCOMPLETE] * (m - n)
    assert [r.size for r in recs[:n]] == [30 + k for k in range(n)]


# ---- overflow ----
def test_overflow_goes_to_the_serial_kernel(eng, ser, cases):
    c = cases["overflow"]
    assert c.serial and sm.nodes(c.stream) > sm.node_cap(c.max_frames, len(c.stream))
    run_case(eng, ser, c)                                                      # (both engines report the serial kernel)


# ---- the call's own checks ----
def test_arguments(eng):
    L = _ffi.lib()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    off = torch.zeros(4, dtype=torch.int64, device=DEV)
    for bad in ((eng.h, None, 10, 3, off.data_ptr(), None), (eng.h, buf.data_ptr(), 10, 3, None, None)):
        r = L.lz4f_mi355x_dev_splitFrames(*bad)
        assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
    assert L.lz4f_mi355x_dev_splitFrames(eng.h, None, 0, 0, None, None) == 0   # max_frames == 0: nothing to do
    one = torch.full((1,), OFF_PAT, dtype=torch.int64, device=DEV)
    eng.split_frames_async(buf, 0, one)
    eng.stream.synchronize()
    assert one.item() == OFF_PAT
    for args in ((buf, 3, off[:3]), (buf, -1, off), (buf, True, off), (buf, 3, off.cpu()), (buf, 3, off.to(torch.int32)), (buf.to(torch.int8), 3, off),
                 (buf, 3, off, buf[:31]), (buf.cpu(), 3, off)):
        with pytest.raises(ValueError):
            eng.split_frames_async(*args)


# ---- nothing of an earlier call leaks into the next ----
def test_smaller_stream_after_a_larger_one(eng, ser, cases):
    for e, path in ((eng, PARALLEL), (ser, SERIAL)):
        for name in ("depth/2051", "short", "false/nested", "stop/at_once", "short"):
            c = cases[name]
            assert run_split(e, c.stream, len(c.planted.starts) + 1)[0] == path
        stream, a = sm.truncation_stream()
        assert run_split(e, stream[:a + 9], 2)[0] == path
        assert run_split(e, stream, 2)[0] == path


# ---- the chains ----
@pytest.fixture(scope="module")
def corpus():
    """About 300 records of 0 to 4096 bytes - the phrase dictionary's natural records and stitched ones - and an input of 200 KiB."""
    d = dc.dictionary("phrase")
    src = dc.tail(d)
    recs = [x for _, x in dc.natural("phrase") if len(x) <= 4096]
    r = dc.rng_of("split/corpus")
    for k in range(300 - len(recs)):
        recs.append(dc.stitched("split/%d" % k, int(r.integers(0, 4097)), src))
    recs.insert(40, dc.stitched("split/big0", 200 << 10, src, (1500, 6000)))
    return d, recs


@pytest.mark.parametrize("directory", [False, True])
def test_chain_compress_pack_split_measure_decode(eng, corpus, directory):
    """One stream, no synchronisation until the end.  The split reads the whole destination buffer (how long the stream is, only the
    device knows): the walk stops at the filler behind the last frame, and consumed says where."""
    d, inputs = corpus
    n = len(inputs)
    p = conduit.make_preferences(blockSizeID=4, blockMode=1)
    lens = [len(x) for x in inputs]
    d_dict = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(DEV)
    d_in = torch.from_numpy(np.frombuffer(b"".join(inputs), dtype=np.uint8).copy()).to(DEV)
    in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(DEV)
    do = frame_windows(lens, p, 3)
    win = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    win_off = torch.tensor(do, dtype=torch.int64, device=DEV)
    out = torch.full((win.numel() + pack_directory_size(n),), PAT, dtype=torch.uint8, device=DEV)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    src_off = torch.full((n + 1,), OFF_PAT, dtype=torch.int64, device=DEV)
    res, srec, mres, dres = eng.new_results(n), eng.new_results(1), eng.new_results(n), eng.new_results(n)
    dst_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    dst = torch.full((sum(lens) + 4096,), PAT, dtype=torch.uint8, device=DEV)   # (no frame here needs more than its size: whole blocks)
    with eng.create_cdict(d_dict) as cd:
        eng.compress_frames_async(d_in, in_off, win, win_off, p, res, cdict=cd)
        eng.pack_frames_async(win, win_off, res, out, out_off, directory=directory)
        eng.split_frames_async(out, n, src_off, record=srec)
        eng.measure_frames_async(out, src_off, mres, dst_off)
        eng.decompress_frames_async(out, src_off, dst, dst_off, dres, dictionary=cd)
        got = eng.frame_results(dres)                                          # the one wait
    assert all(r.status == 0 for r in eng.frame_results(res))
    assert torch.equal(src_off, out_off)
    total = int(out_off[-1].item())
    r = eng.frame_results(srec)[0]
    assert (r.status, r.consumed, r.n_blocks, r.first_bad_block) == (sm.ST_FRAMETYPE, total, n, n) and r.flags >> 12 == PARALLEL
    assert r.size == total - (pack_directory_size(n) if directory else 0) and bool(r.flags & sm.FLAG_SKIPPABLE) == directory
    do2, host = dst_off.cpu().tolist(), dst.cpu().numpy()
    assert do2[-1] == sum(lens)
    for i, x in enumerate(inputs):
        assert got[i].status == 0 and got[i].size == len(x), i
        assert host[do2[i]:do2[i] + len(x)].tobytes() == x, i
    assert (host[do2[-1]:] == PAT).all()
    assert sm.split(out[:total].cpu().numpy().tobytes(), n)[0] == out_off.cpu().tolist()      # ... and the model agrees on the stream alone


def test_chain_of_oracle_frames_split_and_decoded(eng, ser):
    made = sm.oracle_frames()
    stream = b"".join(f for _, f, _ in made)
    n = len(made)
    for e in (eng, ser):
        _, off, src = run_split(e, stream, n)
        res, dst_off = e.new_results(n), torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        e.measure_frames_async(src, off, res, dst_off)
        e.stream.synchronize()
        dst = torch.full((int(dst_off[-1].item()) + 64,), PAT, dtype=torch.uint8, device=DEV)
        e.decompress_frames_async(src, off, dst, dst_off, res)
        recs = e.frame_results(res)
        do, host = dst_off.cpu().tolist(), dst.cpu().numpy()
        for i, (prefs, f, x) in enumerate(made):
            alone, used = oracle.decompress_frame(f, cap=len(x) + 16)
            assert used == len(f) and alone == x
            assert recs[i].status == 0 and recs[i].consumed == len(f), (i, prefs)
            assert host[do[i]:do[i] + recs[i].size].tobytes() == alone, (i, prefs)
