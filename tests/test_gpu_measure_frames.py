"""lz4f_mi355x_dev_measureFrames (Engine.measure_frames_async): what a batch of frames decodes to, and the windows the batch
decoder needs for them, without decoding.

Every record and every window is held to tests/measure_model.py (itself held to the oracle by tests/test_measure_model_cpu.py);
the measured offsets go into decompress_frames_async untouched; measure and the decoder agree wherever both have a say; a frame
behind a block-table overflow is measured as it is in a roomy batch; a bad frame changes no neighbour's record, and the source's
address changes nothing."""
import numpy as np
import pytest
import torch

import lz4_grammar
import measure_model as mm
from lz4_frame_conduit_amd import conduit, datagen
from lz4_frame_conduit_amd.device import Engine, frame_windows, synth50_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_BATCH = 0x1000
PAT = 0xA5
GUARD = 192


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def fields(r):
    return (r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags & 0x1FF)


def measure(eng, frames, src_gap=0, guards=True, shift=0, pad=0, want_off=True):
    """One measure call: frame i's span is frames[i] and src_gap bytes more, with an empty span in front of each and behind the
    last when `guards`; the source starts `shift` bytes into its allocation and has `pad` spare bytes behind.  The record tensor
    has two records more than the call needs and the offsets four elements more, all filled with a pattern that must survive.
    -> (records of the real frames, their W, the tensors: src, src_off, dst_off, and which entries are the real frames)."""
    so, real = [0], []
    for f in frames:
        if guards:
            so.append(so[-1])
        real.append(len(so) - 1)
        so.append(so[-1] + len(f) + src_gap)
    if guards:
        so.append(so[-1])
    n = len(so) - 1
    blob = np.zeros(shift + so[-1] + pad, dtype=np.uint8)
    for f, k in zip(frames, real):
        blob[shift + so[k]:shift + so[k] + len(f)] = np.frombuffer(f, dtype=np.uint8)
    src = torch.from_numpy(blob).to(DEV)[shift:]
    src_off = torch.tensor(so, dtype=torch.int64, device=DEV)
    res = torch.full(((n + 2) * 32,), PAT, dtype=torch.uint8, device=DEV)
    off_all = torch.full((n + 1 + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=DEV)
    dst_off = off_all[:n + 1]
    eng.measure_frames_async(src, src_off, res[:n * 32], dst_off if want_off else None)
    recs = eng.frame_results(res[:n * 32])
    assert (res[n * 32:].cpu() == PAT).all(), "records beyond n_frames were written"
    assert (off_all[n + 1:].cpu() == -0x5A5A5A5A5A5A5A5B).all(), "offsets beyond n_frames + 1 were written"
    if not want_off:
        assert (off_all.cpu() == -0x5A5A5A5A5A5A5A5B).all()
        return [recs[k] for k in real], None, (src, src_off, None, real)
    do = dst_off.cpu().tolist()
    W = [do[k + 1] - do[k] for k in range(n)]
    assert do[0] == 0 and all(w >= 0 for w in W), "not a prefix sum"
    for k in range(n):
        assert recs[k].flags >> 12 == PATH_BATCH
        if k not in set(real):                                # an empty span: frameHeader_incomplete, no window
            assert fields(recs[k]) == (12, 0, 0, 0, mm.NONE, 0) and W[k] == 0, k
    return [recs[k] for k in real], [W[k] for k in real], (src, src_off, dst_off, real)


def inband_frame(eng):
    data = datagen.synth50(3 << 20, 3)
    src = torch.from_numpy(data).to(DEV)
    p = conduit.make_preferences(blockSizeID=4, blockMode=1)
    fr = torch.zeros(eng.frame_bound_inband(src.numel(), p), dtype=torch.uint8, device=DEV)
    eng.compress_async(src, fr, p, inband=True)
    r = eng.result()
    return fr[:r.size].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def run(eng):
    """The whole corpus measured in one batch, spans three bytes apart, then decoded through the measured offsets as they are."""
    fs = list(mm.frames()) + [("inband_trailer", inband_frame(eng))]
    recs, W, (src, src_off, dst_off, real) = measure(eng, [f for _, f in fs], src_gap=3)
    total = int(dst_off[-1].item())                             # (the one read-back of the pipeline)
    dst = torch.full((total + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    kept = dst_off.clone()
    n = src_off.numel() - 1
    dres = eng.new_results(n)
    eng.decompress_frames_async(src, src_off, dst, dst_off, dres)
    drecs = eng.frame_results(dres)
    assert torch.equal(kept, dst_off)
    do = dst_off.cpu().tolist()
    return dict(fs=fs, recs=recs, W=W, total=total, do=[do[k] for k in real], drecs=[drecs[k] for k in real], dst=dst, tensors=(src, src_off, real))


def test_equal_to_the_model(run):
    n_ok = 0
    for (name, f), r, w in zip(run["fs"], run["recs"], run["W"]):
        m = mm.model_of(f + bytes(3))                               # (the span: the frame and the three bytes to the next one)
        assert fields(r) + (w,) == tuple(m), (name, fields(r) + (w,), tuple(m))
        n_ok += m.status == 0
    assert n_ok > len(run["fs"]) // 3
    assert run["total"] == sum(run["W"])                            # (the guards' windows are empty: measure() checked them)


def test_pipeline_decodes_through_the_measured_windows(run):
    dst, short = run["dst"], {0: 0, 1: 0}
    assert (dst[run["total"]:] == PAT).all()
    n_ok = 0
    for (name, f), r, w, at, d in zip(run["fs"], run["recs"], run["W"], run["do"], run["drecs"]):
        err, want, used = mm.oracle_verdict(f)
        if err is not None:
            continue
        n_ok += 1
        assert d.status == 0 and (d.size, d.consumed) == (len(want), used), (name, fields(d))
        assert dst[at:at + d.size].cpu().numpy().tobytes() == want, name
        if w > r.size:
            short[(r.flags >> 5) & 1] += 1
    assert n_ok > len(run["fs"]) // 3
    assert short[0] >= 4 and short[1] >= 4, short                   # frames of short inner blocks, linked and independent: W > size


def test_agrees_with_the_decoder(eng, run):
    src, src_off, real = run["tensors"]
    # the decoder's say in ample windows: a whole block for every block measure counted
    n = src_off.numel() - 1
    wins = [0] * n
    for (name, f), r, k in zip(run["fs"], run["recs"], real):
        wins[k] = r.n_blocks << (8 + 2 * ((f[5] >> 4) & 7)) if r.n_blocks else 0
    do = np.concatenate([[0], np.cumsum(wins)]).astype(np.int64)
    dst = torch.empty(int(do[-1]) + 64, dtype=torch.uint8, device=DEV)
    dres = eng.new_results(n)
    eng.decompress_frames_async(src, src_off, dst, torch.from_numpy(do).to(DEV), dres)
    ample = eng.frame_results(dres)
    n_ok = 0
    for (name, f), r, k in zip(run["fs"], run["recs"], real):
        d = ample[k]
        if d.status == 0:
            n_ok += 1
            assert fields(r) == fields(d), (name, fields(r), fields(d))
        elif r.status == 0:                                         # what measure does not look at, and nothing else
            assert d.status in (mm.GENERIC, mm.BLOCKCK, mm.CONTENTCK), (name, d.status)
    assert n_ok > len(run["fs"]) // 3
    # the decode into W of what measure accepts: never "too small"
    for (name, f), r, d, k in zip(run["fs"], run["recs"], run["drecs"], real):
        if r.status == 0:
            assert d.status != mm.DSTSMALL, name
            assert d.status == ample[k].status, name


def small_frames():
    fs = {n: f for n, f in mm.frames()}
    names = ["edges/win/exact", "edges/flg/combo/c1d1k1", "grammar/end/sparse/short/M4/k0", "grammar/end/dense/short/M8/k4", "grammar/link/bsid4/hist_10+20+30+40/+0",
             "grammar/lit/cut/short_by_one", "made/b4/i0/k3", "made/b4/i1/k3", "made/b5/i1/k3", "made/empty/b4", "made/skippable_first_k9", "edges/csize/+1",
             "edges/end/no_endmark"]
    return [(n, fs[n]) for n in names]


def test_table_overflow_falls_back_per_frame(eng):
    fr = lz4_grammar.Frame(4)
    for i in range(3000):
        fr.stored(bytes([i & 255]))
    tiny = fr.bytes()
    fs = [("3000 stored bytes", tiny)] + small_frames()
    frames = [f for _, f in fs]
    recs, W, (src, src_off, _, _) = measure(eng, frames)
    n = src_off.numel() - 1
    assert 3000 > n + src.numel() // 256 + 1                       # (the documented bound: the first frame alone overflows the table)
    roomy, Wr, (src2, src_off2, _, _) = measure(eng, frames, pad=4 << 20)
    assert 3000 + 64 < n + src2.numel() // 256 + 1
    for (name, f), a, b, wa, wb in zip(fs, recs, roomy, W, Wr):
        assert fields(a) + (wa,) == fields(b) + (wb,) == tuple(mm.model_of(f)), name
    assert fields(recs[0])[:4] == (0, 3000, len(tiny), 3000) and W[0] == 2999 * 65536 + 1


def test_bad_frames_are_isolated_at_every_address(eng):
    good = small_frames()
    base = dict(mm.frames())["made/b4/i1/k1"]                     # independent 64 KiB blocks with block checksums
    st, flg, consumed, bs, blocks = mm.walk(base)
    assert st == 0 and len(blocks) >= 3
    w1, p1 = blocks[1]
    cuts = [3, 6, 7, blocks[0][1] - 2, blocks[0][1], blocks[0][1] + 100, p1 - 3, p1 - 1, p1 + (w1 & 0x7FFFFFFF) + 2, consumed - 6, consumed - 4, consumed - 1]
    clean, Wc, _ = measure(eng, [f for _, f in good])
    frames, kinds = [], []
    for k in range(max(len(good), len(cuts))):
        if k < len(cuts):
            frames.append(base[:cuts[k]]); kinds.append(("cut", k))
        if k < len(good):
            frames.append(good[k][1]); kinds.append(("good", k))
    ref = None
    for shift in range(16):
        recs, W, _ = measure(eng, frames, shift=shift)
        got = [fields(r) + (w,) for r, w in zip(recs, W)]
        if ref is None:
            ref = got
            for (kind, k), g, f in zip(kinds, got, frames):
                assert g == tuple(mm.model_of(f)), (kind, k)
                if kind == "good":
                    assert g == fields(clean[k]) + (Wc[k],), good[k][0]
                else:
                    assert g[0] == mm.INCOMPLETE and g[6] == 0, (k, g)
        assert got == ref, shift


def test_degenerate_calls(eng):
    # no frames: nothing is enqueued, nothing written
    src = torch.zeros(16, dtype=torch.uint8, device=DEV)
    off = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(src, torch.zeros(1, dtype=torch.int64, device=DEV), eng.new_results(0), off)
    eng.stream.synchronize()
    assert off.item() == 7
    # no offsets wanted: the records are the same
    fs = small_frames()
    a, W, (src, src_off, dst_off, real) = measure(eng, [f for _, f in fs])
    b, _, _ = measure(eng, [f for _, f in fs], want_off=False)
    assert [fields(x) for x in a] == [fields(x) for x in b]
    # offsets out of order and out of extent: that frame alone
    so = src_off.cpu().tolist()
    k1, k2 = real[1], real[4]
    bad = list(so); bad[k1] = so[k1 + 1] + 1                          # frame k1's span reversed (the guard in front of it grows: no matter)
    bad.append(src.numel() + 1)                                       # an extra last frame whose span ends past the source
    n = len(bad) - 1
    res, doff = eng.new_results(n), torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(src, torch.tensor(bad, dtype=torch.int64, device=DEV), res, doff)
    r = eng.frame_results(res)
    d = doff.cpu().tolist()
    assert fields(r[k1]) == (mm.SRCPTR, 0, 0, 0, mm.NONE, 0) and fields(r[n - 1]) == (mm.SRCPTR, 0, 0, 0, mm.NONE, 0)
    assert d[k1 + 1] == d[k1] and d[n] == d[n - 1]
    for j, k in enumerate(real):
        if k != k1:
            assert fields(r[k]) == fields(a[j]) and d[k + 1] - d[k] == W[j], fs[j][0]
    assert k2 != k1


def test_more_blocks_than_the_decoder_takes(eng):
    """The batch decoder refuses a span with more blocks than a fifth of its bytes and two, in any window (empty stored blocks, 4
    bytes each, get there): measure says the same, and gives no window."""
    fs = [mm.empty_stored_frame(n, linked=linked) for linked in (False, True) for n in (3, 21, 22, 60)]
    recs, W, (src, src_off, _, real) = measure(eng, fs)
    n = src_off.numel() - 1
    wins = [0] * n
    for f, k in zip(fs, real):
        wins[k] = (len(f) - 11) // 4 * 65536                      # a whole block for every block
    do = np.concatenate([[0], np.cumsum(wins)]).astype(np.int64)
    dst = torch.empty(int(do[-1]) + 64, dtype=torch.uint8, device=DEV)
    dres = eng.new_results(n)
    eng.decompress_frames_async(src, src_off, dst, torch.from_numpy(do).to(DEV), dres)
    dec = eng.frame_results(dres)
    for f, r, w, k in zip(fs, recs, W, real):
        m = mm.model_of(f)
        assert fields(r) + (w,) == tuple(m), (len(f), fields(r), w, tuple(m))
        assert dec[k].status == r.status, (len(f), dec[k].status, r.status)
        if r.status == 0:
            assert fields(dec[k]) == fields(r)
    assert [r.status for r in recs] == [0, 0, mm.DSTSMALL, mm.DSTSMALL] * 2
    # ... and the accepted ones decode into their measured windows
    recs2, W2, (src, src_off, dst_off, real) = measure(eng, fs)
    dst = torch.empty(int(dst_off[-1].item()) + 64, dtype=torch.uint8, device=DEV)
    dres = eng.new_results(src_off.numel() - 1)
    eng.decompress_frames_async(src, src_off, dst, dst_off, dres)
    dec = eng.frame_results(dres)
    assert [dec[k].status for k in real] == [0, 0, mm.DSTSMALL, mm.DSTSMALL] * 2


def test_many_frames_measure_then_decode(eng):
    """Compress, measure, decode: three one-workgroup scans over the frames in tiles of 1024, with the last tile full, holding one
    frame, and one short of full."""
    for n, fb in ((4096, 4096), (2049, 1024), (2047, 1024)):
        _many_frames_measure_then_decode(eng, n, fb)


def _many_frames_measure_then_decode(eng, n, fb):
    data = synth50_device(n * fb, 7, DEV)
    p = conduit.make_preferences(blockSizeID=4, blockMode=1)
    wo = frame_windows([fb] * n, p)
    so = torch.arange(0, n + 1, dtype=torch.int64, device=DEV) * fb
    co = torch.tensor(wo, dtype=torch.int64, device=DEV)
    comp = torch.zeros(wo[-1], dtype=torch.uint8, device=DEV)
    cres = eng.new_results(n)
    eng.compress_frames_async(data, so, comp, co, p, cres)
    res, doff = eng.new_results(n), torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(comp, co, res, doff)
    out = torch.full((n * fb + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    dres = eng.new_results(n)
    eng.decompress_frames_async(comp, co, out, doff, dres)
    made, meas, dec = eng.frame_results(cres), eng.frame_results(res), eng.frame_results(dres)
    assert torch.equal(doff, so)
    for c, m, d in zip(made, meas, dec):
        assert c.status == 0 and fields(m) == (0, fb, c.size, 1, mm.NONE, m.flags & 0x1FF) and fields(d) == fields(m)
    assert torch.equal(out[:n * fb], data) and (out[n * fb:] == PAT).all()
