"""lz4f_mi355x_dev_packFrames and lz4f_mi355x_dev_readPackDirectory (Engine.pack_frames_async, Engine.read_pack_directory_async):
a batch's frames back to back in one stream, made on the device from the compress call's windows and records, and the stream's own
frame directory turned back into offsets.

Every result - the packed bytes, the offsets and the record - is held to tests/pack_model.py (itself held to the oracle by
tests/test_pack_model_cpu.py).  Pack does not parse, so most cases run on synthetic records over seeded random bytes, with the
lengths chosen exactly: around the 16-byte unit and the copy kernel's tile, runs of empty and of 11-byte frames, every alignment
of source and destination, records that lie, a destination one byte short, forged directories.  Destination, offsets and record
carry guards that must survive.  Two chains with real frames end in the batch decoder and in the oracle."""
import struct

import numpy as np
import pytest
import torch

import dict_cases as dc
import oracle
import pack_model as pm
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd.device import PACK_TILE, DeviceCodecError, Engine, frame_windows, pack_directory_size, peek_pack_directory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT = 0xA5
OFF_PAT = -0x5A5A5A5A5A5A5A5B
GUARD = 192                                  # bytes, a multiple of 16: the views' alignment is their shift
T = PACK_TILE
EDGES = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5]
REC = np.dtype([("size", "<u8"), ("consumed", "<u8"), ("status", "<u4"), ("n_blocks", "<u4"), ("first_bad_block", "<u4"), ("flags", "<u4")])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def synthetic(lengths, seed=1, gaps=(0, 1, 29)):
    """Windows over seeded random bytes: frame i is lengths[i] bytes at the start of a window with gaps[i % 3] bytes behind it.
    -> (src bytes, src_off, records as (status, size))"""
    so = [0]
    for i, n in enumerate(lengths):
        so.append(so[-1] + n + gaps[i % len(gaps)])
    src = np.random.default_rng(seed).integers(0, 256, max(so[-1], 1), dtype=np.uint8).tobytes()
    return src, so, [(0, n) for n in lengths]


def shifted(data: bytes, shift: int) -> torch.Tensor:
    """data in device memory, `shift` bytes past an allocation's (256-byte aligned) start."""
    t = torch.empty(shift + len(data), dtype=torch.uint8, device=DEV)
    t[shift:].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    return t[shift:]


def records_tensor(records) -> torch.Tensor:
    a = np.zeros(len(records), dtype=REC)
    for i, (st, size) in enumerate(records):
        a[i] = (size, 7, st, 1, pm.NONE, 0x60)
    return torch.from_numpy(a.view(np.uint8).copy()).to(DEV)


def rec_of(r) -> pm.Rec:
    return pm.Rec(r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags)


def run_pack(eng, src, src_off, records, directory, dst_bytes=None, src_shift=0, dst_shift=0, want_record=True):
    """One pack call held to the model, guards and all -> (the model's dst, dst_off, record; the destination view)."""
    n = len(records)
    want_dst, want_off, want_rec = pm.pack(src, src_off, records, 1 << 40 if dst_bytes is None else dst_bytes, directory, src_bytes=len(src))
    if dst_bytes is None:
        dst_bytes = want_rec.size + 37
    d_src = shifted(src, src_shift)
    dst_all = torch.full((GUARD + dst_shift + dst_bytes + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    dst = dst_all[GUARD + dst_shift:GUARD + dst_shift + dst_bytes]
    off_all = torch.full((4 + n + 1 + 4,), OFF_PAT, dtype=torch.int64, device=DEV)
    rec_all = torch.full((96,), PAT, dtype=torch.uint8, device=DEV)
    eng.pack_frames_async(d_src, torch.tensor(src_off, dtype=torch.int64, device=DEV), records_tensor(records), dst, off_all[4:4 + n + 1],
                          directory=directory, record=rec_all[32:64] if want_record else None)
    eng.stream.synchronize()
    got_all, got_off, got_rec = dst_all.cpu().numpy(), off_all.cpu().numpy(), rec_all.cpu().numpy()
    assert (got_off[:4] == OFF_PAT).all() and (got_off[4 + n + 1:] == OFF_PAT).all(), "offsets outside the n + 1 were written"
    assert (got_rec[:32] == PAT).all() and (got_rec[64:] == PAT).all(), "bytes around the record were written"
    assert got_off[4:4 + n + 1].tolist() == want_off
    if want_record:
        r = eng.frame_results(rec_all[32:64])[0]
        assert rec_of(r) == want_rec, (rec_of(r), want_rec)
    else:
        assert (got_rec == PAT).all()
    lo = GUARD + dst_shift
    written = len(want_dst) if want_dst is not None else 0
    assert (got_all[:lo] == PAT).all() and (got_all[lo + written:] == PAT).all(), "bytes outside d_dst[0 .. d_dst_off[n]) were written"
    if want_dst is not None:
        assert got_all[lo:lo + written].tobytes() == want_dst
    return want_dst, want_off, want_rec, dst


def edge_lengths():
    return EDGES + [0] * 40 + [11] * 40 + EDGES[::-1] + [5, 0, 0, 27]


@pytest.mark.parametrize("directory", [False, True])
def test_lengths_around_unit_and_tile(eng, directory):
    lengths = edge_lengths()
    src, so, recs = synthetic(lengths)
    dst, off, rec, _ = run_pack(eng, src, so, recs, directory)
    assert rec.status == 0 and rec.consumed == sum(lengths) and rec.n_blocks == sum(1 for x in lengths if x) and rec.first_bad_block == pm.NONE
    assert rec.size > 6 * T                                              # more than one workgroup's tile
    run_pack(eng, src, so, recs, directory, want_record=False)            # the record is optional


@pytest.mark.parametrize("shifts", [(0, 0), (1, 0), (0, 1), (3, 13), (15, 15)])
def test_every_alignment_gives_the_same_bytes(eng, shifts):
    src, so, recs = synthetic(edge_lengths(), seed=2)
    for directory in (False, True):
        run_pack(eng, src, so, recs, directory, src_shift=shifts[0], dst_shift=shifts[1])      # (== the model's bytes: the same at every shift)


def test_scan_carries_across_tiles(eng):
    lengths = [11 if i % 2 == 0 else 1 for i in range(2051)]
    src, so, recs = synthetic(lengths, seed=3)
    for directory in (False, True):
        stream, off, rec, _ = run_pack(eng, src, so, recs, directory, dst_shift=7)
        assert rec.n_blocks == 2051 and off[-1] - off[0] == sum(lengths)
    got, r, _ = read_directory(eng, stream, 2051, shift=1)                 # the directory's scan carries too
    assert r.status == 0 and got.cpu().tolist() == off
    read_directory(eng, stream[:16] + bytes([stream[16] ^ 1]) + stream[17:], 2051)      # ... and is written over when the sums differ


def test_records_that_lie_are_empty_slots(eng):
    lengths = [x for x in edge_lengths() if x != 3 * T + 5]
    src, so, clean = synthetic(lengths, seed=4, gaps=(3, 1, 29))
    n = len(lengths)
    a, b, c, d = 6, 9, 12, n - 1                                          # (frames of 32, 256, T and 27 bytes)
    assert all(lengths[i] > 0 for i in (a, b, c, d))
    recs, off = list(clean), list(so)
    recs[a] = (pm.ST_DSTSMALL, 50)                                        # failed by the encoder, with a size in its record
    recs[b] = (0, so[b + 1] - so[b] + 1)                                  # one byte more than its window
    off[c] = off[c + 1] + 5                                               # descending (frame c - 1's window only grows)
    off[n] = len(src) + 1                                                 # a span that ends past srcBytes
    for directory in (False, True):
        dst, doff, rec, _ = run_pack(eng, src, off, recs, directory)
        assert rec.status == 0 and rec.first_bad_block == b
        empty = {a, b, c, d}
        usable = 0
        for i in range(n):
            got = dst[doff[i]:doff[i + 1]]
            if i in empty:
                assert got == b"", i
            else:                                                         # as in the clean batch
                assert got == src[so[i]:so[i] + lengths[i]], i
                usable += lengths[i] > 0
        assert usable * 2 >= n and rec.n_blocks == usable


def test_room(eng):
    src, so, recs = synthetic(edge_lengths(), seed=5)
    for directory in (False, True):
        total = pm.pack(src, so, recs, 1 << 40, directory)[2].size
        dst, off, rec, _ = run_pack(eng, src, so, recs, directory, dst_bytes=total - 1, dst_shift=3)
        assert dst is None and rec.status == pm.ST_DSTSMALL and rec.size == total and off[-1] == total      # (run_pack: the pattern is intact everywhere)
        dst, off, rec, _ = run_pack(eng, src, so, recs, directory, dst_bytes=total, dst_shift=3)
        assert rec.status == 0 and len(dst) == total


def test_call_errors(eng):
    src, so, recs = synthetic([100, 0, 33], seed=6)
    n = len(recs)
    buf = torch.full((4096,), PAT, dtype=torch.uint8, device=DEV)
    buf[:len(src)].copy_(torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()))
    before = buf.cpu().numpy().copy()
    d_off, d_rec = torch.tensor(so, dtype=torch.int64, device=DEV), records_tensor(recs)
    out_off = torch.full((n + 1,), OFF_PAT, dtype=torch.int64, device=DEV)
    for dst in (buf[len(src) - 1:], buf[:50], buf[10:len(src) - 10]):      # the destination's head in the source; its tail; inside
        with pytest.raises(DeviceCodecError, match="overlaps"):
            eng.pack_frames_async(buf[:len(src)], d_off, d_rec, dst, out_off)
    dst = buf[len(src):]                                                  # touching is not overlapping
    eng.pack_frames_async(buf[:len(src)], d_off, d_rec, dst, out_off)
    eng.stream.synchronize()
    assert dst[:133].cpu().numpy().tobytes() == pm.pack(src, so, recs, 1 << 20, False)[0]
    buf.copy_(torch.from_numpy(before))
    out_off.fill_(OFF_PAT)
    # null pointers, straight through the C ABI: each is the call's error, and nothing is enqueued
    L, args = eng.L, [eng.h, n, buf.data_ptr(), len(src), d_off.data_ptr(), d_rec.data_ptr(), buf.data_ptr() + 2048, 2048, out_off.data_ptr(), 0, None]
    for k in (2, 4, 5, 6, 8):
        bad = list(args)
        bad[k] = None
        r = L.lz4f_mi355x_dev_packFrames(*bad)
        assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC" and b"null pointer" in L.lz4f_mi355x_last_error(), k
    for k in (2, 4):
        bad = [eng.h, n, buf.data_ptr(), 2048, out_off.data_ptr(), None]
        bad[k] = None
        r = L.lz4f_mi355x_dev_readPackDirectory(*bad)
        assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC", k
    # no frames: 0, and nothing happens
    assert L.lz4f_mi355x_dev_packFrames(eng.h, 0, None, 0, None, None, None, 0, None, 1, None) == 0
    assert L.lz4f_mi355x_dev_readPackDirectory(eng.h, 0, None, 0, None, None) == 0
    one = torch.full((1,), OFF_PAT, dtype=torch.int64, device=DEV)
    eng.pack_frames_async(buf[:0], torch.zeros(1, dtype=torch.int64, device=DEV), d_rec[:0], buf[2048:], one, directory=True)
    eng.stream.synchronize()
    assert one.item() == OFF_PAT and (out_off.cpu().numpy() == OFF_PAT).all()
    assert (buf.cpu().numpy() == before).all()
    # what is wrong with the tensors: ValueError
    with pytest.raises(ValueError):
        eng.pack_frames_async(buf[:len(src)], d_off, d_rec, buf[2048:], out_off[:n])
    with pytest.raises(ValueError):
        eng.pack_frames_async(buf[:len(src)], d_off, d_rec[:-1], buf[2048:], out_off)
    with pytest.raises(ValueError):
        eng.pack_frames_async(buf[:len(src)], d_off.cpu(), d_rec, buf[2048:], out_off)
    with pytest.raises(ValueError):
        eng.read_pack_directory_async(buf, n, out_off[:n])


def read_directory(eng, stream: bytes, n: int, shift=0):
    """One directory read held to the model -> (the offsets tensor, the model's record, the stream in device memory)."""
    want_off, want_rec = pm.read_directory(stream, n)
    pack = shifted(stream, shift)
    off_all = torch.full((4 + n + 1 + 4,), OFF_PAT, dtype=torch.int64, device=DEV)
    rec_all = torch.full((96,), PAT, dtype=torch.uint8, device=DEV)
    eng.read_pack_directory_async(pack, n, off_all[4:4 + n + 1], record=rec_all[32:64])
    eng.stream.synchronize()
    got_off, got_rec = off_all.cpu().numpy(), rec_all.cpu().numpy()
    assert (got_off[:4] == OFF_PAT).all() and (got_off[4 + n + 1:] == OFF_PAT).all(), "offsets outside the n + 1 were written"
    assert (got_rec[:32] == PAT).all() and (got_rec[64:] == PAT).all(), "bytes around the record were written"
    assert got_off[4:4 + n + 1].tolist() == want_off
    assert rec_of(eng.frame_results(rec_all[32:64])[0]) == want_rec
    return off_all[4:4 + n + 1], want_rec, pack


def test_directory_round_trip_and_forgeries(eng):
    lengths = EDGES[:12] + [0] * 5 + [11] * 1100 + [300, 0, 7]               # (more than one tile of the scan)
    src, so, recs = synthetic(lengths, seed=7)
    n = len(lengths)
    stream, doff, rec, _ = run_pack(eng, src, so, recs, True, dst_shift=9)
    D, stored, fb = peek_pack_directory(stream[:24])
    assert (D, stored, fb) == (pack_directory_size(n), n, rec.consumed) and D + fb == len(stream)
    off, r, _ = read_directory(eng, stream, stored, shift=5)
    assert r.status == 0 and off.cpu().tolist() == doff                   # exactly the d_dst_off the pack wrote
    read_directory(eng, stream + b"more", n)                              # bytes behind the stream are the receiver's business

    def put32(b, at, v):
        return b[:at] + struct.pack("<I", v & 0xFFFFFFFF) + b[at + 4:]
    len3 = struct.unpack_from("<I", stream, 24 + 12)[0]
    forged = [("magic", put32(stream, 0, pm.DIR_MAGIC ^ 0x40), n), ("tag", put32(stream, 8, pm.DIR_TAG ^ 1), n),
              ("n+1 stored", put32(stream, 12, n + 1), n), ("n-1 stored", put32(stream, 12, n - 1), n),
              ("n+1 asked", stream, n + 1), ("n-1 asked", stream, n - 1),
              ("n+1 stored, payload to match", put32(put32(stream, 12, n + 1), 4, 16 + 4 * (n + 1)), n),
              ("a length + 1", put32(stream, 24 + 12, len3 + 1), n), ("framesBytes + 1", put32(stream, 16, fb + 1), n),
              ("packBytes = D - 1", stream[:D - 1], n), ("packBytes = D + framesBytes - 1", stream[:-1], n), ("23 bytes", stream[:23], n)]
    seen = set()
    for what, b, nn in forged:
        off, r, pack = read_directory(eng, b, nn, shift=3)
        assert r.status != 0 and not off.cpu().any(), what
        seen.add(r.status)
    assert seen == {pm.ST_INCOMPLETE, pm.ST_FRAMETYPE, pm.ST_FRAMESIZE}
    # the batch decoder, given those zeros: frameHeader_incomplete for every frame, and no output byte
    off, _, pack = read_directory(eng, put32(stream, 16, fb + 1), n)
    dst = torch.full((64 * n,), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(n)
    eng.decompress_frames_async(pack, off, dst, torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device=DEV), res)
    assert all((x.status, x.size) == (pm.ST_INCOMPLETE, 0) for x in eng.frame_results(res))
    assert (dst == PAT).all()


def test_equal_bytes(eng):
    lengths = edge_lengths()
    src, so, recs = synthetic(lengths, seed=8)
    first, doff, _, view = run_pack(eng, src, so, recs, True, dst_shift=11)
    again, _, _, _ = run_pack(eng, src, so, recs, True, dst_shift=11)
    assert first == again
    for i in (0, 11, 12, 14, 60, len(lengths) - 1):                       # a frame packed alone is the bytes it has in the batch
        alone, _, _, _ = run_pack(eng, src, so[i:i + 2], recs[i:i + 1], False, dst_shift=i % 16)
        assert alone == first[doff[i]:doff[i + 1]], i


# ---- the chains, with real frames ----
def fields(r):
    return (r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags)


@pytest.fixture(scope="module")
def corpus():
    """About 300 records of 0 to 4096 bytes - the phrase dictionary's natural records and stitched ones - and two inputs of 200 KiB."""
    d = dc.dictionary("phrase")
    src = dc.tail(d)
    recs = [x for _, x in dc.natural("phrase") if len(x) <= 4096]
    r = dc.rng_of("pack/corpus")
    for k in range(300 - len(recs)):
        recs.append(dc.stitched("pack/%d" % k, int(r.integers(0, 4097)), src))
    recs.insert(40, dc.stitched("pack/big0", 200 << 10, src, (1500, 6000)))
    recs.append(dc.stitched("pack/big1", 200 << 10, src, (1500, 6000)))
    return d, recs


def compress_batch(eng, inputs, p, failed, **how):
    """compress_frames_async into frame_windows, the window of `failed` deliberately too small -> (windows, their offsets, records)"""
    lens = [len(x) for x in inputs]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    do = frame_windows(lens, p, 3)
    cut = (do[failed + 1] - do[failed]) - 10
    assert lens[failed] >= 500
    do = do[:failed + 1] + [x - cut for x in do[failed + 1:]]             # ten bytes for a record of 500 and more
    joined = b"".join(inputs)
    d_in = torch.from_numpy(np.frombuffer(joined, dtype=np.uint8).copy()).to(DEV)
    win = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    win_off = torch.tensor(do, dtype=torch.int64, device=DEV)
    res = eng.new_results(len(inputs))
    eng.compress_frames_async(d_in, torch.from_numpy(so).to(DEV), win, win_off, p, res, **how)
    return win, win_off, res


def test_chain_compress_pack_directory_measure_decode(eng, corpus):
    d, inputs = corpus
    n, failed = len(inputs), next(i for i, x in enumerate(inputs) if 500 <= len(x) <= 4096)
    p = conduit.make_preferences(blockSizeID=4, blockMode=1)
    d_dict = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(DEV)
    with eng.create_cdict(d_dict) as cd:
        win, win_off, res = compress_batch(eng, inputs, p, failed, cdict=cd)                                  # 1
        out = torch.full((win.numel() + pack_directory_size(n),), PAT, dtype=torch.uint8, device=DEV)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        prec = eng.new_results(1)
        eng.pack_frames_async(win, win_off, res, out, out_off, directory=True, record=prec)                   # 2
        pr = eng.frame_results(prec)[0]                                                                       # 3: the one read-back
        assert pr.status == 0 and pr.n_blocks == n - 1 and pr.first_bad_block == pm.NONE
        recv_all = torch.full((5 + pr.size,), PAT, dtype=torch.uint8, device=DEV)
        recv = recv_all[5:]
        recv.copy_(out[:pr.size])
        assert (out[pr.size:] == PAT).all()
        D, stored, fb = peek_pack_directory(recv[:24].cpu().numpy().tobytes())                                # 4
        assert stored == n and D + fb == pr.size
        src_off = torch.zeros(stored + 1, dtype=torch.int64, device=DEV)
        eng.read_pack_directory_async(recv, stored, src_off)                                                  # 5
        mres, dst_off = eng.new_results(n), torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        eng.measure_frames_async(recv, src_off, mres, dst_off)                                                # 6
        total = int(dst_off[-1].item())
        assert total == sum(len(x) for i, x in enumerate(inputs) if i != failed)
        dst = torch.full((total + GUARD,), PAT, dtype=torch.uint8, device=DEV)
        dres = eng.new_results(n)
        eng.decompress_frames_async(recv, src_off, dst, dst_off, dres, dictionary=cd)                         # 7
        got = eng.frame_results(dres)
        assert torch.equal(src_off, out_off)
        # decoding the unpacked windows directly, into the same windows of output
        dst2 = torch.full((total + GUARD,), PAT, dtype=torch.uint8, device=DEV)
        dres2 = eng.new_results(n)
        eng.decompress_frames_async(win, win_off, dst2, dst_off, dres2, dictionary=cd)
        direct = eng.frame_results(dres2)
    crecs = eng.frame_results(res)
    assert crecs[failed].status == pm.ST_DSTSMALL and sum(1 for x in crecs if x.status) == 1
    do, host = dst_off.cpu().tolist(), dst.cpu().numpy()
    for i, x in enumerate(inputs):                                                                            # 8
        if i == failed:
            assert (got[i].status, got[i].size) == (pm.ST_INCOMPLETE, 0) and do[i] == do[i + 1]
            continue
        assert got[i].status == 0 and got[i].size == len(x) and got[i].consumed == crecs[i].size, i
        assert host[do[i]:do[i] + len(x)].tobytes() == x, i
        assert fields(got[i]) == fields(direct[i]), i
    assert (host[total:] == PAT).all()


def test_chain_without_dictionary_decodes_with_the_oracle(eng, corpus):
    _, inputs = corpus
    inputs = inputs[30:110]                                                # (one of the 200 KiB inputs among them)
    n, failed = len(inputs), next(i for i, x in enumerate(inputs) if 500 <= len(x) <= 4096)
    p = conduit.make_preferences(blockSizeID=4, blockMode=0, contentChecksum=1)
    win, win_off, res = compress_batch(eng, inputs, p, failed)
    out = torch.full((win.numel(),), PAT, dtype=torch.uint8, device=DEV)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    prec = eng.new_results(1)
    eng.pack_frames_async(win, win_off, res, out, out_off, record=prec)
    pr = eng.frame_results(prec)[0]
    assert pr.status == 0 and pr.n_blocks == n - 1 and out_off[0].item() == 0
    stream = out[:pr.size].cpu().numpy().tobytes()
    outs, pos = [], 0
    while pos < len(stream):                                               # a concatenated .lz4 stream: frame after frame
        o, used = oracle.decompress_frame(stream[pos:pos + (1 << 19)], cap=1 << 18)
        outs.append(o)
        pos += used
    assert pos == len(stream)
    assert outs == [x for i, x in enumerate(inputs) if i != failed]
