"""Every decode entry point on frames with TWO flaws (tests/flaw_pairs.py): which flaw decides.

The drop-in surfaces - LZ4F_decompress whole and in pieces, conduit.decompress, conduit.decompressBatched - have no order of their
own: they must give liblz4's recorded answer (tests/golden/flaw_pairs.json), liblz4's bytes for the clean frames, and no success
where liblz4 only waits for more input or room.  The one-shot calls - lz4f_mi355x_decompressFrame, Engine.decompress_frame_async
under every switch set, decompress_blocks_async with a caller's table, decompress_frames_async plain, with a dictionary and with a
dictionary set - must give the status and first_bad_block of flaw_pairs.one_shot_verdict, the order written down in
include/lz4f_mi355x.h ("WHICH FLAW DECIDES"), in the content's window, five bytes more and every block's full room, with guard
bytes around every window.  Engine.measure_frames_async is held to tests/measure_model.py on the same frames.  Every test prints
what it compared and every disagreement before it asserts; the closing test asserts which decoders and block counts the corpus
reached."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import dict_cases as dc
import flaw_pairs as fp
import measure_model as mm
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_frame_conduit_amd.device import Engine
from test_gpu_batch_frames import DEV, GUARD, PAT, PATH_BATCH, _dev
from test_gpu_grammar import ENVS, PATH
from test_gpu_measure_frames import fields, measure

pytestmark = pytest.mark.gpu
SEEN = collections.Counter()            # path bit -> records that carried it
BLOCKS_SEEN = collections.Counter()     # (entry point, shape, n_blocks of a record whose walk came through) -> records
COUNTS = collections.Counter()          # entry point -> comparisons


@pytest.fixture(scope="module")
def L():
    lib = _ffi.lib()
    assert lib.lz4f_mi355x_device_count() >= 1, "these tests need the MI355X"
    return lib


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    fx = fp.load_fixture()["cases"]
    out = fp.cases()
    for c in out:
        assert fp.sha(c.frame) == fx[c.name]["frame_sha256"], c.name          # the generator still makes the minted frames
    return out


@pytest.fixture(scope="module")
def fx():
    return fp.load_fixture()["cases"]


def report(what, bad):
    print("%s: %d disagreements" % (what, len(bad)))
    for b in bad:
        print("   ", *b)


def saw(entry, shape, rec):
    for k, v in PATH.items():
        if (rec.flags >> 12) & v: SEEN[k] += 1
    if (rec.flags >> 12) & PATH_BATCH: SEEN["batch"] += 1
    if rec.n_blocks: BLOCKS_SEEN[entry, shape, rec.n_blocks] += 1


# ---- the drop-in surfaces --------------------------------------------------------------------------------------------------------
def without_room(c, fx):
    """The recorded answer for a surface that has no window: the case's, without its room flaw."""
    if c.room is None: return fx[c.name]
    rest = "+".join(fp._flaw_name(f) for f in c.flaws if f[0] != "room") or "clean"
    return fx["%s/%s/%s" % (c.shape, c.mode, rest)]


def conduit_word(call, frame: bytes) -> str:
    try:
        return "OK:" + fp.sha(b"".join(call([frame])))
    except conduit.Lz4FrameError as e:
        msg = str(e)
        if msg.startswith("lz4frame error: "):
            return fp.ref_verdict({"error": msg[len("lz4frame error: "):], "stall": None})
        return "STALL_input" if "stream ended before EndMark" in msg else "OTHER:" + msg


def differs(got: str, want: str) -> bool:
    """A drop-in's answer against liblz4's: the same word; where liblz4 only waits, anything but success."""
    return got.startswith("OK:") if want.startswith("STALL_") else got != want


def test_drop_ins_give_liblz4s_answer(L, cases, fx):
    bad = []
    for c in cases:
        budget = fp.room_window(c, False) if c.room is not None else fp.ample(c)
        feeds = [("LZ4F_decompress whole", "once", None)]
        if c.shape == "short5": feeds.append(("LZ4F_decompress pieces", "pieces", fp.pieces_seed(c)))
        for entry, key, seed in feeds:
            got, want = fp.ref_verdict(fp.feed(L, c.frame, budget, seed)), fp.ref_verdict(fx[c.name][key])
            COUNTS[entry] += 1
            if differs(got, want): bad.append((c.name, entry, got, want))
        want = fp.ref_verdict(without_room(c, fx)["once"])
        for entry, call in (("conduit.decompress", conduit.decompress), ("conduit.decompressBatched", conduit.decompressBatched)):
            got = conduit_word(call, c.frame)
            COUNTS[entry] += 1
            if differs(got, want): bad.append((c.name, entry, got, want))
    report("drop-ins against liblz4", bad)
    assert not bad, (len(bad), bad[:20])


# ---- the one-shot calls ----------------------------------------------------------------------------------------------------------
def host_call(L, frame: bytes, cap: int) -> int:
    """lz4f_mi355x_decompressFrame into cap bytes with guards on both sides -> the status number."""
    buf = ctypes.create_string_buffer(bytes([PAT]) * (GUARD + cap + GUARD), GUARD + cap + GUARD)
    used = ctypes.c_size_t(0)
    r = L.lz4f_mi355x_decompressFrame(ctypes.byref(buf, GUARD), cap, frame, len(frame), ctypes.byref(used))
    raw = buf.raw
    assert raw[:GUARD] == raw[GUARD + cap:] == bytes([PAT]) * GUARD, "bytes outside the capacity were written"
    return (1 << 64) - r if L.LZ4F_isError(r) else 0


def size_words_walk(frame: bytes):
    """[(payload position, size word)] of a frame whose size words walk to the EndMark inside the span, else None."""
    pos, out, n = 7 + (8 if frame[4] & 8 else 0), [], len(frame)
    while True:
        if n - pos < 4: return None
        w = int.from_bytes(frame[pos:pos + 4], "little"); pos += 4
        if w == 0: return out if n - pos >= 4 else None
        if (w & 0x7FFFFFFF) > fp.BS or n - pos < (w & 0x7FFFFFFF) + 4: return None
        out.append((pos, w)); pos += (w & 0x7FFFFFFF) + 4


def table_call(eng, frame: bytes, blocks):
    """decompress_blocks_async with the caller's table (block i at i * maxBlockSize, every block's full room) -> the record."""
    cap = len(blocks) * fp.BS
    ent = np.zeros(len(blocks) + 1, dtype=np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("word", "<u4"), ("dst_size", "<u4")]))
    for i, (p, w) in enumerate(blocks):
        ent[i] = (p, i * fp.BS, w, fp.BS)
    back = torch.full((GUARD + cap + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    tb = torch.from_numpy(np.frombuffer(ent.tobytes(), dtype=np.uint8).copy()).to(DEV)
    info = _ffi.FrameInfo()
    info.blockSizeID, info.blockMode, info.blockChecksumFlag = (frame[5] >> 4) & 7, (frame[4] >> 5) & 1, (frame[4] >> 4) & 1
    eng.decompress_blocks_async(_dev(frame, 32), len(frame), back[GUARD:GUARD + cap], tb, len(blocks), info)
    rec = eng._result()
    assert bool((back[:GUARD] == PAT).all()) and bool((back[GUARD + cap:] == PAT).all()), "bytes outside the capacity were written"
    return rec, back[GUARD:GUARD + rec.size].cpu().numpy().tobytes() if rec.status == 0 else None


def test_host_pointer_call(L, cases, fx):
    """lz4f_mi355x_decompressFrame: the written order with the blocks back to back (it gives no block a provisional place)."""
    rows = []
    for c in cases:
        for w in fp.windows(c, False):
            st = host_call(L, c.frame, w)
            rows.append((c.name + " @%d" % w, "lz4f_mi355x_decompressFrame", (st, 0), (fp.one_shot_verdict(c, w, placed=False)[0], 0), False))
    COUNTS["lz4f_mi355x_decompressFrame"] += len(rows)
    bad = fp.disagreements(rows)
    report("host-pointer call against the written order", bad)
    assert not bad, (len(bad), bad[:20])


def test_table_call(eng, cases, fx):
    """decompress_blocks_async has no walk, no content size and no content checksum: the blocks in order, and nothing else."""
    rows = []
    for c in cases:
        blocks = size_words_walk(c.frame)
        if blocks is None or c.room is not None: continue
        rec, out = table_call(eng, c.frame, blocks)
        saw("table", c.shape, rec)
        of_blocks = [f for f in fp.failures(c.frame, len(blocks) * fp.BS) if f[1] != fp.NONE]
        rows.append((c.name, "decompress_blocks_async", (rec.status, rec.first_bad_block), of_blocks[0] if of_blocks else (0, fp.NONE), c.mode == "linked"))
        if rec.status == 0 and not c.flaws:
            assert "OK:" + fp.sha(out) == fp.ref_verdict(fx[c.name]["once"]), c.name
    COUNTS["decompress_blocks_async"] += len(rows)
    bad = fp.disagreements(rows)
    report("table call against the written order", bad)
    assert not bad, (len(bad), bad[:20])
    assert len(rows) >= 200                                           # (the cases without a word flaw, a truncation or a room: 220)


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=["+".join(k[len("LZ4F_MI355X_"):] + ("=" + v if v != "1" else "") for k, v in e.items()) or "default" for e in ENVS])
def test_single_call_under_every_switch_set(L, cases, fx, ei):
    """Engine.decompress_frame_async (lz4f_mi355x_dev_decompressFrame) with a fresh engine per switch set.  The stated exception is
    asserted as what it says: for a malformed linked frame the same status and a first_bad_block not in front of the model's.
    The edge shapes get every window under the default switches and every block's full room - the one window in which their walk
    comes through - under the others."""
    env = ENVS[ei]
    rows = []
    os.environ.update(env)
    L.lz4f_mi355x_release_engines()
    try:
        e = Engine(0)
        for c in cases:
            wins = fp.windows(c, True)
            if ei and c.shape.startswith("edge"): wins = wins[-1:]
            for w in wins:
                got, out = single_call(e, c.frame, w)
                saw("single", c.shape, got)
                rows.append((c.name + " @%d" % w, "decompress_frame_async", (got.status, got.first_bad_block), fp.one_shot_verdict(c, w), c.mode == "linked"))
                if got.status == 0:
                    assert "OK:" + fp.sha(out) == fp.ref_verdict(fx[c.name]["once"]), c.name
        e.close()
    finally:
        for k in env: os.environ.pop(k, None)
        L.lz4f_mi355x_release_engines()
    COUNTS["decompress_frame_async"] += len(rows)
    bad = fp.disagreements(rows)
    report("single call under %s against the written order" % (env or "{}"), bad)
    assert not bad, (len(bad), bad[:20])


def single_call(eng, frame: bytes, cap: int):
    """lz4f_mi355x_dev_decompressFrame into cap bytes with guards on both sides -> (record, the output of an accepted frame)."""
    f = _dev(frame)
    d = torch.full((GUARD + cap + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    r = eng.L.lz4f_mi355x_dev_decompressFrame(eng.h, ctypes.c_void_p(d.data_ptr() + GUARD), cap, ctypes.c_void_p(f.data_ptr()), len(frame),
                                               ctypes.c_void_p(eng._res.data_ptr()))
    assert not eng.L.LZ4F_isError(r), "no header flaw here: the call itself never fails"
    rec = eng._result()
    assert bool((d[:GUARD] == PAT).all()) and bool((d[GUARD + cap:] == PAT).all()), "bytes outside the capacity were written"
    return rec, d[GUARD:GUARD + rec.size].cpu().numpy().tobytes() if rec.status == 0 else None


def run_batch(eng, frames, wins, **how):
    """One decompress_frames_async call: frame i in a window of wins[i] bytes, a guard gap - the window of an empty span - in front of
    each and behind the last -> (records of the frames, the destination as bytes, where each window starts)."""
    so, do, real = [0], [0], []
    for f, w in zip(frames, wins):
        so.append(so[-1]); do.append(do[-1] + GUARD)
        real.append(len(so) - 1)
        so.append(so[-1] + len(f)); do.append(do[-1] + w)
    so.append(so[-1]); do.append(do[-1] + GUARD)
    src = _dev(b"".join(frames), 64)
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(so) - 1)
    if "dictset" in how: how = dict(how, slots=torch.zeros(len(so) - 1, dtype=torch.int32, device=DEV))
    eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), res, **how)
    recs = eng.frame_results(res)
    out = dst.cpu().numpy().tobytes()
    isreal = set(real)
    for k in range(len(recs)):
        if k not in isreal:
            assert recs[k].status == fp.INCOMPLETE and out[do[k]:do[k + 1]] == bytes([PAT]) * GUARD, ("a guard gap was written", k)
    return [recs[k] for k in real], out, [do[k] for k in real]


def rec_fields(r):
    return (r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags)


@pytest.mark.parametrize("how", ["plain", "dictionary", "dictset"])
def test_batch_call(eng, cases, fx, how):
    """decompress_frames_async: every case in each of its windows, a clean frame after every eighth flawed one.  The clean
    frames' records and bytes are those of a batch of the clean frames alone, a second run gives the same records, and a frame in
    a batch names the first bad block, linked or not."""
    d1k = _dev(dc.dictionary("d1k"))
    cd = eng.create_cdict(d1k) if how == "dictset" else None
    ds = eng.create_dictset([cd], [7]) if how == "dictset" else None
    kw = {"plain": {}, "dictionary": {"dictionary": d1k}, "dictset": {"dictset": ds}}[how]
    good = [c for c in cases if not c.flaws]
    flawed = [c for c in cases if c.flaws]
    assert len(good) == 12
    alone, aout, ado = run_batch(eng, [g.frame for g in good], [g.n_blocks * fp.BS for g in good], **kw)
    for g, r, at in zip(good, alone, ado):
        assert r.status == 0 and "OK:" + fp.sha(aout[at:at + r.size]) == fp.ref_verdict(fx[g.name]["once"]), g.name
    rows = []
    for k in range(3):
        mix, wins = [], []
        for i, c in enumerate(flawed):
            ws = fp.windows(c, True)
            mix.append(c); wins.append(ws[min(k, len(ws) - 1)])
            if i % 8 == 7:
                g = good[(i // 8) % len(good)]
                mix.append(g); wins.append(g.n_blocks * fp.BS)
        recs, out, do = run_batch(eng, [c.frame for c in mix], wins, **kw)
        again, _, _ = run_batch(eng, [c.frame for c in mix], wins, **kw)
        assert [rec_fields(r) for r in recs] == [rec_fields(r) for r in again], "two runs of one batch gave other records"
        for c, w, r, at in zip(mix, wins, recs, do):
            assert r.flags >> 12 == PATH_BATCH, (c.name, hex(r.flags))
            saw("batch", c.shape, r)
            if c.flaws:
                rows.append((c.name + " @%d" % w, "decompress_frames_async " + how, (r.status, r.first_bad_block), fp.one_shot_verdict(c, w), False))
            else:
                a = alone[good.index(c)]
                assert rec_fields(r) == rec_fields(a) and out[at:at + r.size] == aout[ado[good.index(c)]:ado[good.index(c)] + a.size], ("a good neighbour changed", c.name)
            assert out[at + w:at + w + GUARD] == bytes([PAT]) * GUARD, ("bytes behind the window were written", c.name)
    if ds is not None: ds.close()
    if cd is not None: cd.close()
    COUNTS["decompress_frames_async " + how] += len(rows)
    bad = fp.disagreements(rows)
    report("batch call (%s) against the written order" % how, bad)
    assert not bad, (len(bad), bad[:20])


def test_measure_call(eng, cases):
    """Engine.measure_frames_async on the same frames, against tests/measure_model.py: it looks at no checksum and no window, so
    bck, cck and room are no flaws to it, and of two flaws it sees the first one it can see."""
    recs, W, _ = measure(eng, [c.frame for c in cases])
    bad = []
    for c, r, w in zip(cases, recs, W):
        m = mm.measure(c.frame)
        if fields(r) + (w,) != tuple(m): bad.append((c.name, fields(r) + (w,), tuple(m)))
    COUNTS["measure_frames_async"] += len(cases)
    report("measure call against its model", bad)
    assert not bad, (len(bad), bad[:20])


def test_what_the_corpus_reached():
    """Run behind the tests above (the whole file): the decoders the path bits name, and the block counts on both sides of the
    one-wave finish (at most 64 blocks) and the finish behind k_finish_check (65 and more)."""
    print("comparisons per entry point:")
    for k, v in sorted(COUNTS.items()):
        print("    %-40s %d" % (k, v))
    print("path bits:", dict(SEEN))
    print("block counts of the edge shapes:", {k: v for k, v in BLOCKS_SEEN.items() if k[1].startswith("edge")})
    assert COUNTS["decompress_frame_async"] and COUNTS["decompress_blocks_async"] and COUNTS["decompress_frames_async plain"], "run the whole file"
    assert SEEN["table"] and SEEN["wave_per_block"] and SEEN["batch"], dict(SEEN)
    assert SEEN["self_index"] or SEEN["indexed"], dict(SEEN)
    for shape, n in (("edge64", 64), ("edge65", 65), ("edge130", 130)):
        assert BLOCKS_SEEN["single", shape, n] > 0, (shape, dict(BLOCKS_SEEN))      # (the single call's finish is what the counts divide)
