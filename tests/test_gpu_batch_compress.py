"""lz4f_mi355x_dev_compressFrames (Engine.compress_frames_async): many inputs, one frame each, in one call.

A frame in a batch must be, byte for byte, the frame lz4f_mi355x_dev_compressFrame writes for that input alone on an engine in
deterministic mode with the same preferences (contentSize = the input's length where the batch was asked for content sizes), with
that call's size, consumed, status, n_blocks and FLG byte; the path bits say PATH_BATCH.  Nothing may be written outside a frame's
window or beyond its size, and a frame that fails (window too small, bad offsets) fails alone."""
import numpy as np
import pytest
import torch

import oracle
from alignment_cases import DST_RES, SRC_RES, carve
from lz4_frame_conduit_amd import conduit, datagen
from lz4_frame_conduit_amd.device import Engine, frame_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_BATCH = 0x1000
GUARD = 192
PAT = 0xA5
NONE = 0xFFFFFFFF
ST_SRC_TOO_LARGE, ST_DST_SMALL, ST_SRC_WRONG = 10, 11, 15


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def det():
    """The reference: the single call on an engine in deterministic mode."""
    e = Engine(0)
    e.set_deterministic(True)
    yield e
    e.close()


_DATA = {}


def data(kind: str) -> bytes:
    if not _DATA:
        _DATA["s50"] = datagen.synth50(9 << 20, 41).tobytes()
        _DATA["text"] = datagen.synth_text(2 << 20, 23).tobytes()
        _DATA["rand"] = datagen.random_bytes(1 << 20, 5).tobytes()
    return _DATA[kind]


def prefs(bsid=4, linked=0, bck=0, cck=0, csize=0, dictid=0, level=0):
    return conduit.make_preferences(blockSizeID=bsid, blockMode=0 if linked else 1, blockChecksum=bck, contentChecksum=cck,
                                    contentSize=1 if csize else 0, dictID=dictid, compressionLevel=level)


def single_prefs(p, n: int):
    """The batch's preferences as the single call takes them for an input of n bytes."""
    q = conduit.make_preferences(blockSizeID=p.frameInfo.blockSizeID, blockMode=p.frameInfo.blockMode, blockChecksum=p.frameInfo.blockChecksumFlag,
                                 contentChecksum=p.frameInfo.contentChecksumFlag, contentSize=n if p.frameInfo.contentSize else 0,
                                 dictID=p.frameInfo.dictID, compressionLevel=p.compressionLevel)
    return q


def _dev(b, extra: int = 0) -> torch.Tensor:
    a = np.frombuffer(bytes(b) + b"\0" * extra, dtype=np.uint8) if len(b) + extra else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a.copy()).to(DEV)


def _off(v) -> torch.Tensor:
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


class Batch:
    """One batch call over `inputs` (bytes each), laid out one behind the other in the source; window i is the frame bound of
    input i plus `gap` guard bytes unless `windows` gives its size.  The destination is PAT before the call."""

    def __init__(self, eng, inputs, p, gap=GUARD, windows=None):
        self.inputs = inputs
        lens = [len(x) for x in inputs]
        so = [0]
        for n in lens:
            so.append(so[-1] + n)
        self.src, self.so = _dev(b"".join(inputs), extra=16), so
        if windows is None:
            do = frame_windows(lens, p, gap)
        else:
            do = [0]
            for w in windows:
                do.append(do[-1] + w)
        self.do = do
        self.dst = torch.full((max(do[-1], 1),), PAT, dtype=torch.uint8, device=DEV)
        self.res = eng.new_results(len(lens))
        self.so_t, self.do_t = _off(self.so), _off(self.do)
        eng.compress_frames_async(self.src, self.so_t, self.dst, self.do_t, p, self.res)
        self.recs = eng.frame_results(self.res)

    def frame(self, i) -> torch.Tensor:
        return self.dst[self.do[i]:self.do[i] + self.recs[i].size]

    def frame_bytes(self, i) -> bytes:
        return self.frame(i).cpu().numpy().tobytes()


def single(det, src: torch.Tensor, p):
    """lz4f_mi355x_dev_compressFrame on this input alone, deterministic mode -> (record, the frame on the device)."""
    n = src.numel() if src is not None else 0
    s = src if n else torch.zeros(1, dtype=torch.uint8, device=DEV)[:0]
    q = single_prefs(p, n)
    cap = det.frame_bound(n, q)
    dst = torch.full((cap + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    det.compress_async(s, dst[:cap], q)
    rec = det._result()
    assert bool((dst[cap:] == PAT).all())
    return rec, dst[:rec.size]


def assert_same(got, want, name):
    assert got.flags >> 12 == PATH_BATCH, (name, hex(got.flags))
    assert got.first_bad_block == NONE, (name, got.first_bad_block)
    a = (got.status, got.size, got.consumed, got.n_blocks, got.flags & 0xFF)
    b = (want.status, want.size, want.consumed, want.n_blocks, want.flags & 0xFF)
    assert a == b, (name, a, b)
    assert not got.flags & 0x200, (name, "ENC_POOL_SHORT in a batch")


def check_identity(b: Batch, det, p, which=None):
    for i in (range(len(b.inputs)) if which is None else which):
        n = len(b.inputs[i])
        want, frame = single(det, b.src[b.so[i]:b.so[i] + n], p)
        assert_same(b.recs[i], want, "input %d (%d bytes)" % (i, n))
        assert want.status == 0 and torch.equal(b.frame(i), frame), "input %d (%d bytes): the frame differs from the single call's" % (i, n)


def check_guards(b: Batch):
    """Everything in a window beyond the frame's size still holds the pattern (frames that succeeded)."""
    for i, r in enumerate(b.recs):
        if r.status == 0:
            tail = b.dst[b.do[i] + r.size:b.do[i + 1]]
            assert bool((tail == PAT).all()), "frame %d wrote beyond its size" % i


def edge_inputs(bs: int, level: int):
    """Inputs at the grammar's and the geometry's edges, and a few hundred KiB to a few MiB of each kind of data."""
    s50, text, rand = data("s50"), data("text"), data("rand")
    out = [text[100:100 + n] for n in (0, 1, 4, 5, 12, 13, 64, 4096)]
    out += [s50[7:7 + n] for n in (65535, 65536, 65537)]
    out += [(s50 if k % 2 else text + s50)[k:k + n] for k, n in enumerate((bs - 1, bs, bs + 1))]
    shrink = 4 if level >= 9 else 1                              # (level 9 does 0.46 GiB/s)
    out += [s50[1 << 20:(1 << 20) + ((2 << 20) + 12345) // shrink], text[:((1 << 20) + 777) // shrink], rand[:((300 << 10) + 1) // shrink],
            (rand + text)[(1 << 20) - 70000:(1 << 20) + 200000 // shrink]]
    return out


FLAGSETS = {"plain": dict(), "bck": dict(bck=1), "cck_csize": dict(cck=1, csize=1), "all_dict": dict(bck=1, cck=1, csize=1, dictid=0x1234ABCD)}


@pytest.mark.parametrize("level", [0, 3, 9])
@pytest.mark.parametrize("flags", list(FLAGSETS))
@pytest.mark.parametrize("linked", [0, 1])
@pytest.mark.parametrize("bsid", [4, 5, 6, 7])
def test_identity_with_the_single_call(eng, det, bsid, linked, flags, level):
    p = prefs(bsid=bsid, linked=linked, level=level, **FLAGSETS[flags])
    b = Batch(eng, edge_inputs(1 << (8 + 2 * bsid), level), p)
    check_identity(b, det, p)
    check_guards(b)


def mixed_inputs():
    s50, text, rand = data("s50"), data("text"), data("rand")
    return [b"", text[:1], s50[:70000], text[:300000], rand[:100000], b"abc" * 50000, s50[:(1 << 20) + 5], text[5:18], bytes(300), rand[:65536]]


@pytest.mark.parametrize("kw", [dict(bsid=4), dict(bsid=5, linked=1, bck=1, cck=1, csize=1), dict(bsid=4, linked=1, level=3), dict(bsid=6, bck=1, dictid=7, level=4)])
def test_frames_are_lz4_frames(eng, kw):
    p = prefs(**kw)
    ins = mixed_inputs()
    b = Batch(eng, ins, p, gap=7)
    for i, x in enumerate(ins):
        assert b.recs[i].status == 0 and b.recs[i].consumed == len(x), (i, b.recs[i].status)
        out, used = oracle.decompress_frame(b.frame_bytes(i), cap=len(x) + 64)
        assert used == b.recs[i].size and out == x, "frame %d does not decode to its input" % i
    # encode -> decode on the device: the encoder's windows are the decoder's spans as they are
    wo = [0]
    for x in ins:
        wo.append(wo[-1] + len(x) + 3)
    back = torch.full((wo[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(ins))
    eng.decompress_frames_async(b.dst, b.do_t, back, _off(wo), res)
    r = eng.frame_results(res)
    for i, x in enumerate(ins):
        assert r[i].status == 0 and r[i].size == len(x) and r[i].consumed == b.recs[i].size, (i, r[i].status, r[i].size)
        assert torch.equal(back[wo[i]:wo[i] + len(x)], b.src[b.so[i]:b.so[i] + len(x)]), i
        assert bool((back[wo[i] + len(x):wo[i + 1]] == PAT).all())


@pytest.mark.parametrize("kw", [dict(bsid=4, bck=1, cck=1), dict(bsid=5, linked=1, level=3)])
def test_isolation(eng, det, kw):
    p = prefs(**kw)
    ins = mixed_inputs()
    first = Batch(eng, ins, p)
    assert all(r.status == 0 for r in first.recs)
    check_guards(first)
    check_identity(first, det, p, which=(0, 2, 6))
    # windows one byte short of the frame for every third frame (sizes from the first run): they fail alone
    short = [i for i in range(len(ins)) if i % 3 == 1]
    wins = [first.recs[i].size - 1 if i in short else first.recs[i].size + GUARD for i in range(len(ins))]
    b = Batch(eng, ins, p, windows=wins)
    out = b.dst.cpu().numpy()
    mask = np.ones(len(out), dtype=bool)
    for i in range(len(ins)):
        if i in short:
            assert (b.recs[i].status, b.recs[i].size) == (ST_DST_SMALL, 0), (i, b.recs[i].status, b.recs[i].size)
            assert b.recs[i].flags >> 12 == PATH_BATCH
            mask[b.do[i]:b.do[i + 1]] = False                       # (bytes inside a failed frame's window are unspecified)
        else:
            assert_same(b.recs[i], first.recs[i], "neighbour %d" % i)
            assert torch.equal(b.frame(i), first.frame(i)), i
            mask[b.do[i]:b.do[i] + b.recs[i].size] = False
    assert (out[mask] == PAT).all(), "bytes outside the frames were written"
    # an exact window suffices
    b = Batch(eng, ins, p, windows=[r.size for r in first.recs])
    for i in range(len(ins)):
        assert_same(b.recs[i], first.recs[i], "exact %d" % i)
        assert torch.equal(b.frame(i), first.frame(i)), i


def test_bad_offsets_fail_alone(eng):
    p = prefs(bsid=4, bck=1)
    ins = mixed_inputs()[:6]
    n = len(ins)
    good = Batch(eng, ins, p)
    so, do = list(good.so), list(good.do)
    # span 1 reversed (it starts behind its end), window 3 reversed, and an extra last frame whose span ends past the source buffer
    so2 = list(so); so2[1] = so[2] + 1
    do2 = list(do); do2[3] = do[4] + 1
    so2.append(good.src.numel() + 1); do2.append(do2[-1] + 64)
    dst = torch.full((do2[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(n + 1)
    eng.compress_frames_async(good.src, _off(so2), dst, _off(do2), p, res)
    r = eng.frame_results(res)
    assert (r[1].status, r[3].status, r[n].status) == (ST_SRC_WRONG, ST_DST_SMALL, ST_SRC_WRONG), [x.status for x in r]
    assert all(x.size == 0 and x.flags >> 12 == PATH_BATCH for x in (r[1], r[3], r[n]))
    out = dst.cpu().numpy()
    mask = np.ones(len(out), dtype=bool)
    for k in (4, 5):                                                # (untouched neighbours: the same frames)
        assert_same(r[k], good.recs[k], "neighbour %d" % k)
        assert torch.equal(dst[do2[k]:do2[k] + r[k].size], good.frame(k)), k
    for k in (0, 2, 4, 5):                                          # (frame 0's span and frame 2's window grew by the reversals: valid, other frames)
        assert r[k].status == 0, (k, r[k].status)
        mask[do2[k]:do2[k] + r[k].size] = False
    assert (out[mask] == PAT).all(), "bytes were written where no valid window lies"
    # the last window ends past the destination buffer
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    do5 = list(do[:n]) + [dst.numel() + 1]
    res = eng.new_results(n)
    eng.compress_frames_async(good.src, _off(so), dst, _off(do5), p, res)
    r = eng.frame_results(res)
    assert r[n - 1].status == ST_DST_SMALL and all(x.status == 0 for x in r[:n - 1]), [x.status for x in r]
    assert bool((dst[do[n - 1]:] == PAT).all()), "a frame whose window is out of extent wrote"
    for k in range(n - 1):
        assert torch.equal(dst[do[k]:do[k] + r[k].size], good.frame(k)), k


def test_call_level_errors_and_no_frames(eng):
    src = _dev(b"x" * 16)
    dst = torch.full((64,), PAT, dtype=torch.uint8, device=DEV)
    z = torch.zeros(1, dtype=torch.int64, device=DEV)
    eng.compress_frames_async(src, z, dst, z, prefs(), eng.new_results(0))
    eng.stream.synchronize()
    assert bool((dst == PAT).all())
    bad = prefs(); bad.frameInfo.blockSizeID = 3
    with pytest.raises(Exception, match="maxBlockSize_invalid"):
        eng.compress_frames_async(src, _off([0, 16]), dst, _off([0, 64]), bad, eng.new_results(1))
    # NULL prefs: the defaults (64 KiB blocks)
    res = eng.new_results(1)
    so, do = _off([0, 16]), _off([0, 64])
    r = eng.L.lz4f_mi355x_dev_compressFrames(eng.h, 1, src.data_ptr(), 16, so.data_ptr(), dst.data_ptr(), 64, do.data_ptr(), None, res.data_ptr())
    assert not eng.L.LZ4F_isError(r)
    rec = eng.frame_results(res)[0]
    assert rec.status == 0 and oracle.decompress_frame(dst[:rec.size].cpu().numpy().tobytes(), cap=64)[0] == b"x" * 16


@pytest.mark.parametrize("kw", [dict(bsid=4, cck=1, csize=1), dict(bsid=5, linked=1, bck=1, level=3)])
def test_order_and_repetition(eng, det, kw):
    p = prefs(**kw)
    ins = mixed_inputs()
    b1 = Batch(eng, ins, p)
    perm = [int(k) for k in np.random.default_rng(11).permutation(len(ins))]
    b2 = Batch(eng, [ins[k] for k in perm], p, gap=5)
    for j, k in enumerate(perm):
        assert_same(b2.recs[j], b1.recs[k], "permuted %d" % k)
        assert torch.equal(b2.frame(j), b1.frame(k)), k
    # a fresh engine, and one that has run other compress and decompress calls before
    fresh = Engine(0)
    try:
        b3 = Batch(fresh, ins, p)
    finally:
        fresh.close()
    check_identity(b1, det, prefs(**kw), which=(2, 3))           # (`det` has compressed; now it decodes, then runs the batch itself)
    back = torch.empty(len(ins[3]) + 64, dtype=torch.uint8, device=DEV)
    det.decompress_frame_async(b1.frame(3), b1.recs[3].size, back)
    assert det._result().size == len(ins[3])
    b4 = Batch(det, ins, p)
    for i in range(len(ins)):
        for other in (b3, b4):
            assert_same(other.recs[i], b1.recs[i], "repeated %d" % i)
            assert torch.equal(other.frame(i), b1.frame(i)), i
    # an input named twice (overlapping spans) gives the same frame twice.  The workspace is sized by the source buffer's extent, which
    # spans that do not overlap cannot exceed: here the buffer holds as much again behind the input, so both get their entries
    n = 200000
    src = _dev(data("s50")[:2 * n + 64])
    so = [0, n, 0, n]                                              # spans 0 and 2 are the input; span 1 is reversed
    do = frame_windows([n, 0, n], p, GUARD)
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(3)
    eng.compress_frames_async(src, _off(so), dst, _off(do), p, res)
    r = eng.frame_results(res)
    assert (r[0].status, r[1].status, r[2].status) == (0, ST_SRC_WRONG, 0) and r[0].size == r[2].size
    assert torch.equal(dst[do[0]:do[0] + r[0].size], dst[do[2]:do[2] + r[2].size])
    want, frame = single(det, src[:n], p)
    assert_same(r[0], want, "twice")
    assert torch.equal(dst[do[0]:do[0] + r[0].size], frame)
    # in a buffer of the input's own extent the second naming finds no entries left: it fails alone, the first is the same frame
    dst.fill_(PAT)
    res = eng.new_results(3)
    eng.compress_frames_async(src[:n], _off(so), dst, _off(do), p, res)
    r = eng.frame_results(res)
    assert (r[0].status, r[1].status, r[2].status, r[2].size) == (0, ST_SRC_WRONG, ST_SRC_TOO_LARGE, 0)
    assert torch.equal(dst[do[0]:do[0] + r[0].size], frame) and bool((dst[do[0] + r[0].size:] == PAT).all())


@pytest.mark.parametrize("kw", [dict(bsid=4, bck=1, cck=1, csize=1), dict(bsid=5, linked=1), dict(bsid=4, linked=1, level=3)])
def test_alignment(eng, kw):
    p = prefs(**kw)
    ins = [x for x in mixed_inputs() if len(x)] + [data("text")[9:9 + 65537], data("s50")[3:3 + 131073]]
    for turn, (sres, dres) in enumerate(zip(SRC_RES[1::3], DST_RES[1:] * 3)):
        # spans at odd addresses: an odd number of filler bytes behind every input, the buffer itself at residue sres.  Span k ends where
        # span k+1 starts, so the filler is part of the input: the frames to compare with are those of an aligned batch over the same spans
        so = [0]
        for k, x in enumerate(ins):
            so.append(so[-1] + len(x) + (2 * ((k + turn) % 5) + 1))
        host = np.full(so[-1], 0x33 + turn, dtype=np.uint8)
        for x, a in zip(ins, so):
            host[a:a + len(x)] = np.frombuffer(x, dtype=np.uint8)
        ref = Batch(eng, [bytes(host[so[k]:so[k + 1]]) for k in range(len(ins))], p)
        assert all(r.status == 0 for r in ref.recs)
        do = [0]                                                    # windows likewise: the frame and an odd number of bytes, at residue dres
        for k in range(len(ins)):
            do.append(do[-1] + ref.recs[k].size + 2 * ((k + 2 * turn) % 7) + 1)
        src, s_front, s_back = carve(so[-1], sres, device=DEV)
        dst, d_front, d_back = carve(do[-1], dres, device=DEV)
        assert src.data_ptr() % 64 == sres and dst.data_ptr() % 64 == dres
        src.copy_(torch.from_numpy(host))
        res = eng.new_results(len(ins))
        eng.compress_frames_async(src, _off(so), dst, _off(do), p, res)
        r = eng.frame_results(res)
        for k in range(len(ins)):
            assert_same(r[k], ref.recs[k], "residues %d/%d input %d" % (sres, dres, k))
            assert torch.equal(dst[do[k]:do[k] + r[k].size], ref.frame(k)), (sres, dres, k)
            assert bool((dst[do[k] + r[k].size:do[k + 1]] == PAT).all()), (sres, dres, k)
        assert bool((s_front == PAT).all() and (s_back == PAT).all() and (d_front == PAT).all() and (d_back == PAT).all())


@pytest.mark.parametrize("n, size, kw", [(4096, 64 << 10, dict(bsid=4)), (65536, 4 << 10, dict(bsid=4, linked=1, bck=1)), (4096, 64 << 10, dict(bsid=4, level=3, cck=1, csize=1))])
def test_many_frames(eng, det, n, size, kw):
    p = prefs(**kw)
    total = n * size
    half = datagen.synth50(total // 2, 3)
    src = torch.from_numpy(np.concatenate([half, datagen.synth_text(total - total // 2, 8)])).to(DEV)
    so = _off(range(0, total + 1, size))
    do = frame_windows([size] * n, p, 0)
    do_t = _off(do)
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(n)
    eng.compress_frames_async(src, so, dst, do_t, p, res)
    recs = eng.frame_results(res)
    assert all(r.status == 0 and r.consumed == size and r.n_blocks == 1 and r.flags >> 12 == PATH_BATCH for r in recs)
    assert sum(r.size for r in recs) < total
    # decoded by the batch decoder straight from the encoder's buffers, compared with the source on the device
    back = torch.zeros(total, dtype=torch.uint8, device=DEV)
    res2 = eng.new_results(n)
    eng.decompress_frames_async(dst, do_t, back, so, res2)
    r2 = eng.frame_results(res2)
    assert all(r.status == 0 and r.size == size for r in r2)
    assert torch.equal(back, src)
    for i in (0, 1, n // 3, n // 2, n // 2 + 1, n - 2, n - 1):      # a sample against the single call - the loop is what this call is there to avoid
        want, frame = single(det, src[i * size:(i + 1) * size], p)
        assert_same(recs[i], want, "frame %d" % i)
        assert torch.equal(dst[do[i]:do[i] + recs[i].size], frame), i
