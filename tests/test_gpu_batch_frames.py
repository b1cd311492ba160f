"""lz4f_mi355x_dev_decompressFrames (Engine.decompress_frames_async): many frames in one call.

A frame in a batch must decode exactly as it does alone through lz4f_mi355x_dev_decompressFrame on the same span and window
(status, size, consumed, n_blocks, first_bad_block, flags & 0x1FF; the path bits say PATH_BATCH; where the single call rejects
the header on the host, its error code is the batch record's status), a frame must not touch anything outside its window, and
a bad frame must not change any other frame's result or bytes."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN_DIR
from lz4_frame_conduit_amd import datagen
from lz4_frame_conduit_amd.device import Engine
from lz4_grammar import corpus

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_BATCH = 0x1000
GUARD = 192
PAT = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _dev(b: bytes, extra: int = 0) -> torch.Tensor:
    a = np.frombuffer(bytes(b) + b"\0" * extra, dtype=np.uint8) if len(b) + extra else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a.copy()).to(DEV)


def single(eng, frame: bytes, cap: int):
    """lz4f_mi355x_dev_decompressFrame on this span and window alone -> (record or LZ4F error code, output bytes or None)."""
    f = _dev(frame)
    d = torch.full((cap + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    r = eng.L.lz4f_mi355x_dev_decompressFrame(eng.h, ctypes.c_void_p(d.data_ptr()), cap, ctypes.c_void_p(f.data_ptr()), len(frame),
                                               ctypes.c_void_p(eng._res.data_ptr()))
    if eng.L.LZ4F_isError(r):
        return (1 << 64) - r, None
    rec = eng._result()
    out = d.cpu().numpy().tobytes()
    assert out[cap:] == bytes([PAT]) * GUARD
    return rec, out[:rec.size] if rec.status == 0 else None


def batch(eng, frames, caps, src_gap=0, dst_gap=GUARD):
    """One batch call: frame i's span is frames[i] (spans src_gap bytes apart), its window caps[i] bytes.  Windows are
    consecutive in the offsets, so the guard gaps of PAT between them are the windows of frames of their own, with empty spans
    (frameHeader_incomplete: nothing may be written for them).  -> (records of the real frames, the whole destination as bytes,
    where each real frame's span starts, where its window starts)."""
    so, do, real = [0], [0], []
    for f, c in zip(frames, caps):
        so.append(so[-1]); do.append(do[-1] + dst_gap)                           # the guard in front
        real.append(len(so) - 1)
        so.append(so[-1] + len(f) + src_gap); do.append(do[-1] + c)
    so.append(so[-1]); do.append(do[-1] + dst_gap)                               # the guard behind the last window
    blob = bytearray(so[-1] + 64)
    for f, k in zip(frames, real):
        blob[so[k]:so[k] + len(f)] = f
    src = _dev(bytes(blob))
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(so) - 1)
    eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), res)
    recs = eng.frame_results(res)
    out = dst.cpu().numpy().tobytes()
    is_real = set(real)
    for k in range(len(recs)):
        if k not in is_real:
            assert recs[k].status == 12 and out[do[k]:do[k + 1]] == bytes([PAT]) * (do[k + 1] - do[k]), k
    return [recs[k] for k in real], out, [so[k] for k in real], [do[k] for k in real]


def out_of(recs, dst, dst_off, i):
    return dst[dst_off[i]:dst_off[i] + recs[i].size]


def assert_same(got, want, name):
    """A batch record against the single call's (record or host error code)."""
    assert got.flags >> 12 == PATH_BATCH, (name, hex(got.flags))
    if isinstance(want, int):
        assert got.status == want, (name, got.status, want)
        return
    a = (got.status, got.size, got.consumed, got.n_blocks, got.first_bad_block, got.flags & 0x1FF)
    b = (want.status, want.size, want.consumed, want.n_blocks, want.first_bad_block, want.flags & 0x1FF)
    if got.status == want.status != 0 and not (want.flags & 0x20) and got.first_bad_block < want.first_bad_block:
        # A malformed LINKED frame: the batch names the first block that does not decode in its own block's room, as liblz4 and
        # the single call's wave decoder do; the single call's linked-frame kernels may name a later one (stated in the header)
        a, b = a[:4] + a[5:], b[:4] + b[5:]
    assert a == b, (name, a, b)


def oracle_out(frame: bytes):
    try:
        return oracle.decompress_frame(frame, cap=max(64 << 20, len(frame) * 300))[0]
    except oracle.OracleError:
        return None


def skippable(payload: bytes) -> bytes:
    return (0x184D2A50).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload


def made_frames():
    """Oracle-made frames over every framing this decoder has to follow."""
    s50 = datagen.synth50(2 << 20, 77).tobytes()
    txt = datagen.synth_text(1 << 20, 5).tobytes()
    out = []
    for bsid in (4, 5, 6, 7):
        for indep in (0, 1):
            for k, (bck, cck, csize, dictid, af) in enumerate([(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 1, 0, 0), (1, 1, 0, 7, 1)]):
                data = (s50 if (bsid + k) % 2 else txt)[: (300 << 10) * (1 + k) + 123 * bsid]
                p = oracle.mkprefs(bsid=bsid, indep=indep, bck=bck, cck=cck, csize=len(data) if csize else 0, dictid=dictid, autoflush=af)
                out.append(("made/b%d/i%d/k%d" % (bsid, indep, k), oracle.conduit_compress(data, p, slice_=5000 if af else 16384)))
        out.append(("made/empty/b%d" % bsid, oracle.conduit_compress(b"", oracle.mkprefs(bsid=bsid, cck=1, csize=0))))
    out.append(("made/skippable_first", skippable(b"not a frame" * 7) + out[3][1]))
    out.append(("made/empty_skippable", skippable(b"")))
    return out


def inband_frame(eng):
    from lz4_frame_conduit_amd import conduit
    data = datagen.synth50(3 << 20, 3)
    src = torch.from_numpy(data).to(DEV)
    p = conduit.make_preferences(blockSizeID=4, blockMode=1)
    fr = torch.zeros(eng.frame_bound_inband(src.numel(), p), dtype=torch.uint8, device=DEV)
    eng.compress_async(src, fr, p, inband=True)
    r = eng.result()
    return fr[:r.size].cpu().numpy().tobytes(), data.tobytes()


def all_frames(eng):
    fs = [(n, f) for n, f, _ in corpus()]
    fs += [("golden/" + os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.lz4")))]
    fs += made_frames()
    fr, _ = inband_frame(eng)
    fs.append(("inband_trailer", fr))
    return fs


def window_for(frame: bytes, k: int) -> int:
    o = oracle_out(frame)
    base = len(o) if o is not None else 4 * len(frame) + 64
    return [base, base + 17, base + (64 << 10)][k % 3]


def test_equal_to_the_single_call(eng):
    fs = all_frames(eng)
    caps = [window_for(f, k) for k, (_, f) in enumerate(fs)]
    recs, dst, _, dst_off = batch(eng, [f for _, f in fs], caps, src_gap=3)
    n_ok = 0
    for i, ((name, f), cap) in enumerate(zip(fs, caps)):
        want, wout = single(eng, f, cap)
        assert_same(recs[i], want, name)
        if recs[i].status == 0:
            n_ok += 1
            got = out_of(recs, dst, dst_off, i)
            assert got == wout, name
            o = oracle_out(f)
            assert o is not None and got == o, name
    assert n_ok > len(fs) // 2
    # every guard gap between the windows untouched
    for i in range(len(fs)):
        assert dst[dst_off[i] + caps[i]:dst_off[i] + caps[i] + GUARD] == bytes([PAT]) * GUARD, fs[i][0]


def _hsize(f):
    flg = f[4]
    return 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)


def test_bad_frames_are_isolated(eng):
    s50 = datagen.synth50(1 << 20, 9).tobytes()
    good = []
    for k, p in enumerate([oracle.mkprefs(bsid=4, indep=1), oracle.mkprefs(bsid=4, indep=0, bck=1), oracle.mkprefs(bsid=5, indep=1, cck=1),
                           oracle.mkprefs(bsid=4, indep=1, bck=1, cck=1), oracle.mkprefs(bsid=6, indep=0)]):
        d = s50[k * 1000: k * 1000 + (200 << 10) + k * 4321]
        good.append((oracle.conduit_compress(d, p), d))
    gcap = [len(d) + 100 for _, d in good]
    base = good[3][0]                                               # bck + cck, independent 64 KiB blocks
    bad_hdr = bytearray(base); bad_hdr[_hsize(base) - 1] ^= 0xFF
    bad_bck = bytearray(base); bad_bck[len(base) - 9] ^= 0x01          # (last block's checksum: in front of the EndMark and the content checksum)
    bad_cck = bytearray(base); bad_cck[-1] ^= 0x01
    cmap = {n: f for n, f, _ in corpus()}
    bad = [(base[:len(base) // 2], len(good[3][1]), {12}), (bytes(bad_hdr), len(good[3][1]), {17}), (bytes(bad_bck), len(good[3][1]), {7}),
           (bytes(bad_cck), len(good[3][1]), {18}), (cmap["off/reach/first/L4/+1"], 1 << 16, {1}), (cmap["off/reach/mid/L4/+1"], 1 << 18, {1}),
           (base, len(good[3][1]) - 1, {11}), (good[4][0], len(good[4][1]) - 5000, {11}), (b"\x04\x22\x4d", 100, {12})]
    clean, cdst, _, cdoff = batch(eng, [f for f, _ in good], gcap)
    for i, (f, d) in enumerate(good):
        assert clean[i].status == 0 and out_of(clean, cdst, cdoff, i) == d
    # interleaved: bad, good, bad, good ...
    frames, caps, kinds = [], [], []
    for k in range(max(len(good), len(bad))):
        if k < len(bad):
            frames.append(bad[k][0]); caps.append(bad[k][1]); kinds.append(("bad", k))
        if k < len(good):
            frames.append(good[k][0]); caps.append(gcap[k]); kinds.append(("good", k))
    recs, dst, _, doff = batch(eng, frames, caps)
    for i, (kind, k) in enumerate(kinds):
        if kind == "good":
            assert_same(recs[i], clean[k], "good %d" % k)
            assert out_of(recs, dst, doff, i) == good[k][1]
        else:
            want, _ = single(eng, bad[k][0], bad[k][1])
            assert_same(recs[i], want, "bad %d" % k)
            assert recs[i].status in bad[k][2], (k, recs[i].status)
    gaps = [dst[doff[i] + caps[i]:doff[i] + caps[i] + GUARD] for i in range(len(frames))] + [dst[:GUARD]]
    assert all(g == bytes([PAT]) * GUARD for g in gaps)
    # offsets out of order and out of extent: those frames get srcPtr_wrong / dstMaxSize_tooSmall and nothing is written for them
    fl = [f for f, _ in good]
    n = len(fl)
    so = [0]
    for f in fl:
        so.append(so[-1] + len(f) + 40)
    do = [GUARD]
    for c in gcap:
        do.append(do[-1] + c + GUARD)
    host = bytearray(so[-1] + 64)
    for f, a in zip(fl, so):
        host[a:a + len(f)] = f
    src = _dev(bytes(host))
    dst = torch.full((do[-1] + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    # frame 1's span reversed (it starts behind the next one's start), frame 3's window reversed, an extra last frame whose span
    # ends past the source buffer
    so2 = list(so); so2[1] = so[2] + 1
    do2 = list(do); do2[3] = do[4] + 1
    so2.append(src.numel() + 1); do2.append(do2[-1])
    res = eng.new_results(n + 1)
    eng.decompress_frames_async(src, torch.tensor(so2, dtype=torch.int64, device=DEV), dst, torch.tensor(do2, dtype=torch.int64, device=DEV), res)
    r = eng.frame_results(res)
    out = np.frombuffer(dst.cpu().numpy().tobytes(), dtype=np.uint8)
    assert (r[1].status, r[3].status, r[n].status) == (15, 11, 15), [x.status for x in r]
    mask = np.ones(len(out), dtype=bool)
    for k in (0, 2, 4):                                            # (frame 0's span and frame 2's window grew by the reversal: no matter)
        assert r[k].status == 0 and out[do2[k]:do2[k] + r[k].size].tobytes() == good[k][1], k
        assert_same(r[k], clean[k], "neighbour %d" % k)
        mask[do2[k]:do2[k + 1]] = False
    assert (out[mask] == PAT).all(), "bytes outside the good frames' windows were written"
    # the last window ends past the destination buffer
    dst.fill_(PAT)
    do5 = list(do[:n]) + [dst.numel() + 1]
    res = eng.new_results(n)
    eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do5, dtype=torch.int64, device=DEV), res)
    r = eng.frame_results(res)
    assert r[n - 1].status == 11 and all(x.status == 0 for x in r[:n - 1]), [x.status for x in r]
    out = np.frombuffer(dst.cpu().numpy().tobytes(), dtype=np.uint8)
    assert (out[do[n - 1]:] == PAT).all(), "a frame whose window is out of extent wrote"


def test_order_does_not_matter(eng):
    fs = made_frames() + [(n, f) for n, f, _ in corpus()[::7]]
    caps = [window_for(f, k) for k, (_, f) in enumerate(fs)]
    r1, d1, _, o1 = batch(eng, [f for _, f in fs], caps)
    perm = np.random.default_rng(11).permutation(len(fs))
    r2, d2, _, o2 = batch(eng, [fs[p][1] for p in perm], [caps[p] for p in perm], src_gap=5)
    for j, p in enumerate(perm):
        assert_same(r2[j], r1[p], fs[p][0])
        if r1[p].status == 0:
            assert out_of(r2, d2, o2, j) == out_of(r1, d1, o1, p), fs[p][0]


def test_zero_and_one_frame(eng):
    src = _dev(b"x" * 16)
    dst = torch.full((64,), PAT, dtype=torch.uint8, device=DEV)
    z = torch.zeros(1, dtype=torch.int64, device=DEV)
    eng.decompress_frames_async(src, z, dst, z, eng.new_results(0))
    assert eng.frame_results(eng.new_results(0)) == []
    assert (dst.cpu() == PAT).all()
    data = datagen.synth50(100 << 10, 1).tobytes()
    f = oracle.conduit_compress(data, oracle.mkprefs(bsid=4, indep=1, bck=1))
    recs, dst, _, doff = batch(eng, [f], [len(data)])
    assert recs[0].status == 0 and recs[0].size == len(data) and recs[0].consumed == len(f) and out_of(recs, dst, doff, 0) == data
    assert recs[0].flags >> 12 == PATH_BATCH


def test_many_tiny_frames_and_empty_windows(eng):
    rng = np.random.default_rng(4)
    kinds = []
    for k in range(50):
        d = bytes(rng.integers(0, 4, size=int(rng.integers(0, 400)), dtype=np.uint8))
        p = oracle.mkprefs(bsid=4, indep=k % 2, bck=(k // 2) % 2, cck=(k // 4) % 2)
        kinds.append((oracle.conduit_compress(d, p), d))
    pick = rng.integers(0, len(kinds), size=10000)
    frames = [kinds[k][0] for k in pick]
    caps = [len(kinds[k][1]) + int(k % 3) for k in pick]
    recs, dst, _, doff = batch(eng, frames, caps, dst_gap=8)
    for i, k in enumerate(pick):
        assert recs[i].status == 0, (i, recs[i].status)
        assert out_of(recs, dst, doff, i) == kinds[k][1]
        assert recs[i].consumed == len(kinds[k][0])
    # zero-length windows: an empty frame decodes into one, a frame with content does not fit
    empty = oracle.conduit_compress(b"", oracle.mkprefs(bsid=4))
    full = kinds[int(np.argmax([len(d) for _, d in kinds]))][0]
    fs = [empty, full, empty, b"", full]
    caps = [0, 0, 0, 0, len(oracle_out(full))]
    recs, dst, _, doff = batch(eng, fs, caps)
    for i, (f, c) in enumerate(zip(fs, caps)):
        want, _ = single(eng, f, c)
        assert_same(recs[i], want, "zero window %d" % i)
    assert [r.status for r in recs] == [0, 11, 0, 12, 0]


def _n_blocks(f):
    flg, pos, n = f[4], _hsize(f), 0
    while True:
        w = int.from_bytes(f[pos:pos + 4], "little")
        if w == 0:
            return n
        pos += 4 + (w & 0x7FFFFFFF) + (4 if flg & 0x10 else 0)
        n += 1


def test_many_short_flushed_blocks(eng):
    """Frames of many short flushed blocks.  As with the single call every block has its provisional place (block i at
    i * maxBlockSize), so such a frame needs a window of n_blocks * maxBlockSize; with less it fails as the single call does."""
    data = datagen.synth_text(300 << 10, 8).tobytes()
    fs = []
    for indep in (0, 1):
        for bck in (0, 1):
            fs.append(oracle.conduit_compress(data, oracle.mkprefs(bsid=4, indep=indep, bck=bck, cck=1, autoflush=1), slice_=300))
    nb = [_n_blocks(f) for f in fs]
    assert min(nb) > 600
    for f in fs:
        assert len(oracle_out(f)) == len(data)
    caps = [nb[0] << 16, (nb[1] << 16) + 1000, len(data), (nb[3] - 1 << 16) + 5]
    recs, dst, _, doff = batch(eng, fs, caps)
    for i, f in enumerate(fs):
        want, wout = single(eng, f, caps[i])
        assert_same(recs[i], want, "short blocks %d" % i)
        if recs[i].status == 0:
            assert recs[i].n_blocks == nb[i] and out_of(recs, dst, doff, i) == data == wout
    assert recs[2].status == 11
    print("many short blocks: statuses", [r.status for r in recs], "first bad", [r.first_bad_block for r in recs])


def test_table_overflow_falls_back_per_frame(eng):
    """Disjoint windows always fit the block table; overlapping ones can overflow it.  Here twelve frames decode into one shared
    window (identical frames: identical bytes), more blocks than the table holds, and the independent frames behind them - short
    blocks in the middle, block and content checksums, a tight last block - are decoded a wave per frame: still exactly as alone."""
    W = 1 << 20
    data = datagen.synth50(W, 21).tobytes()
    A = oracle.conduit_compress(data, oracle.mkprefs(bsid=4, indep=1, bck=1, cck=1))
    m = 12
    cmap = {n: f for n, f, _ in corpus()}
    ts = [(n, cmap[n]) for n in sorted(cmap) if "/short_mid/" in n]
    made = oracle.conduit_compress(data[:300 << 10], oracle.mkprefs(bsid=4, indep=1, bck=1, cck=1))
    ts += [("tight", made), ("exact", made), ("linked", oracle.conduit_compress(data[:200 << 10], oracle.mkprefs(bsid=4, indep=0, bck=1)))]
    caps = [_n_blocks(f) << 16 for _, f in ts[:-3]] + [(300 << 10) - 1, 300 << 10, 200 << 10]
    # entries: A, (reversed), A, (reversed), ..., A, then per test frame a guard (empty span) and the frame, then a guard
    so, do = [0], [0]
    for j in range(m):
        so.append(len(A)); do.append(W)
        if j < m - 1:
            so.append(0); do.append(0)                             # (span and window reversed: srcPtr_wrong)
    host = bytearray(A)
    real = []
    for (_, f), c in zip(ts, caps):
        so.append(so[-1]); do.append(do[-1] + GUARD)
        real.append(len(so) - 1)
        host += f
        so.append(len(host)); do.append(do[-1] + c)
    so.append(so[-1]); do.append(do[-1] + GUARD)
    n = len(so) - 1
    table_cap = n + do[-1] // 65536 + 1
    assert m * _n_blocks(A) > table_cap + 16                       # (the shared window's frames alone overflow the table)
    src = _dev(bytes(host) + bytes(64))
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(n)
    eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), res)
    r = eng.frame_results(res)
    out = dst.cpu().numpy().tobytes()
    assert [x.status for x in r[:2 * m - 1]] == [0, 15] * (m - 1) + [0]
    assert all(x.size == W and x.consumed == len(A) for x in r[:2 * m - 1:2]) and out[:W] == data
    is_real = set(real)
    for k in range(2 * m - 1, n):
        if k not in is_real:
            assert r[k].status == 12 and out[do[k]:do[k + 1]] == bytes([PAT]) * (do[k + 1] - do[k]), k
    statuses = []
    for (name, f), c, k in zip(ts, caps, real):
        want, wout = single(eng, f, c)
        assert_same(r[k], want, name)
        statuses.append(r[k].status)
        if r[k].status == 0:
            o = oracle_out(f)
            assert out[do[k]:do[k] + r[k].size] == wout == o, name
    assert statuses[-3:] == [11, 0, 0] and statuses.count(0) >= len(ts) - 1, statuses


def test_offsets_across_4gib(eng):
    """Spans and windows on both sides of 2^32, and across it."""
    G = 1 << 32
    data = [datagen.synth50(n, n).tobytes() for n in (70 << 10, 300 << 10, 1 << 20)]
    fs = [oracle.conduit_compress(data[0], oracle.mkprefs(bsid=4, indep=1, bck=1)),
          oracle.conduit_compress(data[1], oracle.mkprefs(bsid=4, indep=0, cck=1)),
          oracle.conduit_compress(data[2], oracle.mkprefs(bsid=5, indep=1))]
    so = [G - len(fs[0]) - len(fs[1]) // 2 - 10]
    so += [so[0] + len(fs[0]), so[0] + len(fs[0]) + len(fs[1])]       # frame 1 straddles 2^32, frame 2 lies above it
    so.append(so[-1] + len(fs[2]))
    do = [G - len(data[0]) - len(data[1]) // 2 - 7]
    do += [do[0] + len(data[0]), do[0] + len(data[0]) + len(data[1])]
    do.append(do[-1] + len(data[2]))
    try:
        src = torch.zeros(so[-1] + 64, dtype=torch.uint8, device=DEV)
        dst = torch.full((do[-1] + 64,), PAT, dtype=torch.uint8, device=DEV)
        for f, a in zip(fs, so):
            src[a:a + len(f)] = _dev(f)[:len(f)]
        res = eng.new_results(3)
        eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), res)
        r = eng.frame_results(res)
        for i in range(3):
            assert r[i].status == 0 and r[i].size == len(data[i]) and r[i].consumed == len(fs[i]), (i, r[i].status)
            assert dst[do[i]:do[i + 1]].cpu().numpy().tobytes() == data[i], i
        assert (dst[do[0] - 64:do[0]].cpu() == PAT).all() and (dst[do[-1]:].cpu() == PAT).all()
    finally:
        src = dst = None
        torch.cuda.empty_cache()
