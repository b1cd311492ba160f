"""Every frame decode entry point, and both device encoders' headers, on the frame-edge corpus (tests/frame_edges.py).

Decode: the whole corpus through lz4f_mi355x_dev_decompressFrames (one call), lz4f_mi355x_dev_decompressFrame and the host-pointer
lz4f_mi355x_decompressFrame (a call per case), and lz4f_mi355x_dev_decompressBlocks for the frames the oracle accepts.  A malformed
frame must get the same verdict from all of them, the oracle's; an accepted one the oracle's bytes; nothing may be written outside
a window.  Encode: lz4f_mi355x_dev_compressFrame and lz4f_mi355x_dev_compressFrames must write the oracle's header, and the
same frame."""
import ctypes

import numpy as np
import pytest
import torch

import frame_edges as fe
import oracle
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_frame_conduit_amd.device import Engine, frame_windows
from test_gpu_batch_frames import DEV, GUARD, PAT, _dev, assert_same, batch, single

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    return [(name, f, w, fe.verdict(f, w)) for name, f, w in fe.corpus()]


def code_of(want) -> int:
    """single()'s answer (a record, or the LZ4F error code the call itself returned) -> the status number."""
    return want if isinstance(want, int) else want.status


def host_call(L, frame: bytes, cap: int):
    """lz4f_mi355x_decompressFrame into cap bytes with a guard behind -> (status number, output or None, consumed)."""
    buf = ctypes.create_string_buffer(bytes([PAT]) * (cap + GUARD), cap + GUARD)
    used = ctypes.c_size_t(0)
    r = L.lz4f_mi355x_decompressFrame(buf, cap, frame, len(frame), ctypes.byref(used))
    assert buf.raw[cap:] == bytes([PAT]) * GUARD, "bytes behind the capacity were written"
    if L.LZ4F_isError(r):
        return (1 << 64) - r, None, 0
    return 0, buf.raw[:r], used.value


def table_call(eng, frame: bytes):
    """lz4f_mi355x_dev_decompressBlocks with a table from the Python walk (block i at i * maxBlockSize) -> (record, output)."""
    blocks = fe.blocks_of(frame)
    bs = 1 << (8 + 2 * ((frame[5] >> 4) & 7))
    cap = len(blocks) * bs
    ent = np.zeros(len(blocks) + 1, dtype=np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("word", "<u4"), ("dst_size", "<u4")]))
    for i, (p, w) in enumerate(blocks):
        ent[i] = (p + 4, i * bs, w, bs)
    back = torch.full((cap + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    tb = torch.from_numpy(np.frombuffer(ent.tobytes(), dtype=np.uint8).copy()).to(DEV)
    info = _ffi.FrameInfo()
    info.blockSizeID, info.blockMode, info.blockChecksumFlag = (frame[5] >> 4) & 7, (frame[4] >> 5) & 1, (frame[4] >> 4) & 1
    eng.decompress_blocks_async(_dev(frame, 32), len(frame), back[:cap], tb, len(blocks), info)
    rec = eng._result()
    out = back.cpu().numpy().tobytes()
    assert out[cap:] == bytes([PAT]) * GUARD, "bytes behind the capacity were written"
    return rec, out[:rec.size]


def device_status(f: bytes, w: int, v) -> int:
    """The status the device calls must give: the oracle's, but for the classes pinned here."""
    walks = v.header_ok and not fe.is_skippable(f) and v.error != "ERROR_frameHeader_incomplete" and v.error != "ERROR_maxBlockSize_invalid"
    if walks and any(i * fe.BS >= w for i in range(len(fe.blocks_of(f)))):
        # class "provisional places": the device calls decode block i at i * maxBlockSize and move short blocks together afterwards
        # (lz4f_mi355x.h), so a frame whose size words walk needs window > (n_blocks - 1) * maxBlockSize, whatever its blocks hold:
        # dstMaxSize_tooSmall from the walk.  Oracle: decodes when the window holds the content (win/exact), else
        # dstMaxSize_tooSmall as here.  The host-pointer call has no such rule and is held to the oracle.
        return fe.status_of("ERROR_dstMaxSize_tooSmall")
    return fe.status_of(v.error)


def test_decode_entry_points_agree_with_the_oracle(eng, cases):
    L = eng.L
    recs, dst, _, doff = batch(eng, [f for _, f, _, _ in cases], [w for _, _, w, _ in cases])      # (spans end where the frames end: a cut frame stays cut)
    bad = []
    for i, (name, f, w, v) in enumerate(cases):
        want, wout = single(eng, f, w)
        assert_same(recs[i], want, name)                                      # batch record == single-call record
        st = code_of(want)
        hst, hout, hused = host_call(L, f, w)
        print("%-24s window %6d oracle %-32s single %2d batch %2d host %2d" % (name, w, v.error, st, recs[i].status, hst))
        expect = device_status(f, w, v)
        if st != expect:
            bad.append((name, "status", st, "expected", expect, v.error))
        if hst != (st if expect == fe.status_of(v.error) else fe.status_of(v.error)):
            bad.append((name, "host-pointer status", hst, "single call", st, v.error))
        if v.error is None:
            if hout != v.out or hused != v.consumed:
                bad.append((name, "host-pointer output or consumed", hused, v.consumed))
            if st == 0:
                got = dst[doff[i]:doff[i] + recs[i].size]
                if not (got == wout == v.out):
                    bad.append((name, "output"))
                if not (recs[i].consumed == want.consumed == v.consumed):
                    bad.append((name, "consumed", recs[i].consumed, want.consumed, v.consumed))
            if not fe.is_skippable(f) and fe.blocks_of(f):
                rec, tout = table_call(eng, f)
                if rec.status != 0 or tout != v.out:
                    bad.append((name, "block table call", rec.status))
        # the window's guard in the batch's destination (the single and host calls check their own)
        if dst[doff[i] + w:doff[i] + w + GUARD] != bytes([PAT]) * GUARD:
            bad.append((name, "bytes behind the window were written"))
    assert not bad, (len(bad), bad[:40])
    assert sum(1 for r in recs if r.status == 0) >= 40


SIZES = (0, 1, 70000)


def test_encoders_write_the_oracles_header():
    det = Engine(0)
    det.set_deterministic(True)
    try:
        rng = np.random.default_rng(5)
        body = (bytes(rng.integers(97, 101, size=35000, dtype=np.uint8)) * 2)[:70000]
        for c, d, k in fe.COMBOS:
            p = conduit.make_preferences(blockSizeID=4, blockMode=1, blockChecksum=1, contentChecksum=k, contentSize=1 if c else 0,
                                         dictID=fe.DICT_ID if d else 0, compressionLevel=0)
            datas = [body[:n] for n in SIZES]
            # the batch: every input's frame in its own window, guard gaps between them
            so = [0]
            for x in datas:
                so.append(so[-1] + len(x))
            do = frame_windows([len(x) for x in datas], p, gap=GUARD)
            src = _dev(b"".join(datas))
            dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
            res = det.new_results(len(datas))
            det.compress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), p, res)
            recs = det.frame_results(res)
            out = dst.cpu().numpy().tobytes()
            for j, x in enumerate(datas):
                n = len(x)
                want_head = oracle.header_bytes(fe.combo_prefs(c, d, k, n))
                assert recs[j].status == 0, (c, d, k, n, recs[j].status)
                bframe = out[do[j]:do[j] + recs[j].size]
                assert out[do[j] + recs[j].size:do[j + 1]] == bytes([PAT]) * (do[j + 1] - do[j] - recs[j].size), (c, d, k, n)
                # the single call on this input alone
                q = conduit.make_preferences(blockSizeID=4, blockMode=1, blockChecksum=1, contentChecksum=k, contentSize=n if c else 0,
                                             dictID=fe.DICT_ID if d else 0, compressionLevel=0)
                s = _dev(x)[:n]
                fr = torch.full((det.frame_bound(n, q) + GUARD,), PAT, dtype=torch.uint8, device=DEV)
                det.compress_async(s, fr[:fr.numel() - GUARD], q)
                r = det.result()
                sframe = fr[:r.size].cpu().numpy().tobytes()
                assert bool((fr[r.size:] == PAT).all()), (c, d, k, n)
                assert sframe[:len(want_head)] == want_head, ("single call's header", c, d, k, n, sframe[:20].hex(), want_head.hex())
                assert bframe[:len(want_head)] == want_head, ("batch call's header", c, d, k, n, bframe[:20].hex(), want_head.hex())
                assert bframe == sframe, (c, d, k, n)
                assert oracle.decompress_frame(bframe, cap=n + 64) == (x, len(bframe)), (c, d, k, n)
    finally:
        det.close()
