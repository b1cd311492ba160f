"""Every decoder path against liblz4's verdicts on the LZ4 block grammar's edges (tests/lz4_grammar.py, verdicts recorded
from liblz4 1.9.3 in tests/golden/grammar.json), and on liblz4's HC frames of the project's own sources.

One test per engine switch set that changes which decoder takes a frame without an index; each sends every case through
every decode entry point.  Accepted cases must give liblz4's bytes, rejected ones an error with the bytes behind the
caller's capacity untouched; the verdict must not depend on the capacity once it holds the content (liblz4 judges a block
against its maxBlockSize, whatever room the caller gives).  One deliberate deviation: offset 0, which liblz4 1.9.3 accepts
(the match copies bytes nobody wrote), is rejected everywhere here.

What each entry point gets:
  - lz4f_mi355x_decompressFrame: capacity = content, content + 5, content + maxBlockSize, a guard region behind it;
  - Engine.decompress_frame_async: the same capacities and every block's full room, guarded.  One rule of this call is
    stated, not changed: it decodes every block at its provisional place, block i at i * maxBlockSize, so a frame with a
    short block in the middle needs every block's full room (see test_dense_payloads_in_big_independent_blocks); such
    frames get that room only;
  - decompress_blocks_async: a caller block table (block i at i * maxBlockSize), for every frame whose size words walk;
  - LZ4F_decompress, whole; and in 1..300-byte pieces with 1..500 bytes of room (the feed liblz4's verdict was recorded
    with) for frames up to PIECES_MAX - under the first switch set for all of them, under each other one for every
    len(ENVS)-th case (it is thousands of calls per frame);
  - conduit.decompressBatched.
The sparse full blocks of 256 KiB and 4 MiB that liblz4 accepts must also have been decoded through the self-index, without
the indexed kernels giving up, under the default switches: a stricter check in decode_spx.cuh or in the feeders only sends a
frame to the generic decoders, and that must show too."""
import ctypes
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN_DIR, golden_file
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_grammar import corpus

pytestmark = pytest.mark.gpu
sha = lambda b: hashlib.sha256(b).hexdigest()

# the switch sets that change the decoder of a frame without an index (engine.hip, Switches::read and where each is used)
ENVS = [{}, {"LZ4F_MI355X_NO_SPX": "1"}, {"LZ4F_MI355X_NO_SELFFEED": "1"}, {"LZ4F_MI355X_FEED_ROUND": "24"},
        {"LZ4F_MI355X_DENSE_MODE": "1"}, {"LZ4F_MI355X_DENSE_MODE": "2"}, {"LZ4F_MI355X_SERIAL_WALK": "1"},
        {"LZ4F_MI355X_NO_SELFINDEX": "1"}, {"LZ4F_MI355X_NO_SELFINDEX": "1", "LZ4F_MI355X_NO_WINDOW": "1"},
        {"LZ4F_MI355X_TRACE_ALWAYS": "1"}, {"LZ4F_MI355X_TRACE_ALWAYS": "1", "LZ4F_MI355X_NO_DOUBLING": "1"}]
PATH = dict(table=0x001, parallel_walk=0x004, indexed=0x008, self_index=0x010, doubling=0x020, hops=0x040, window=0x080, fused=0x100,
            wave_per_block=0x200, workgroup_per_block=0x800)
GUARD = 4096
DROPPED = 0x400                  # the indexed kernels gave up and the generic ones decoded
WALK_DELIVERED = 0x2000          # a guessed list of size words was accepted: names no decoder, so not in PATH (tests/test_gpu_walks.py pins it)
PIECES_MAX = 300 << 10           # frames fed in 1..300-byte pieces: up to this size (the rest is thousands of calls each)


@pytest.fixture(scope="module")
def L():
    lib = _ffi.lib()
    assert lib.lz4f_mi355x_device_count() >= 1, "these tests need the MI355X"
    return lib


def _cases():
    with open(os.path.join(GOLDEN_DIR, "grammar.json")) as f:
        g = json.load(f)
    out = []
    for name, frame, meta in corpus():
        rec = g["cases"][name]
        assert sha(frame) == rec["frame_sha256"], name                     # the generator still makes the recorded frames
        ok = rec["once"]["error"] is None and not name.startswith("off/zero/")
        out.append((name, frame, meta, rec["once"]["out_sha256"] if ok else None))
    import lzma
    text = lzma.decompress(golden_file("project_sources.txt.xz"))
    for name, rec in g["hc"].items():
        fr = golden_file(rec["file"])
        assert sha(fr) == rec["frame_sha256"], name
        bs = 1 << (8 + 2 * rec["prefs"]["bsid"])
        out.append(("hc/" + name, fr, dict(bs=bs, linked=not rec["prefs"]["indep"], short_mid=False, content=len(text)), sha(text)))
    return out


def _walk(frame: bytes):
    """The frame's blocks: [(payload offset, size word)] and the position behind the EndMark (None: the walk fails)."""
    flg = frame[4]
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    bs = 1 << (8 + 2 * ((frame[5] >> 4) & 7))
    blocks = []
    while True:
        w = int.from_bytes(frame[pos:pos + 4], "little"); pos += 4
        if w == 0:
            return blocks, pos
        if (w & 0x7FFFFFFF) > bs:
            return blocks, None
        blocks.append((pos, w)); pos += (w & 0x7FFFFFFF) + 4 * ((flg >> 4) & 1)


def host_call(L, frame, cap):
    """lz4f_mi355x_decompressFrame into cap bytes with a guard behind: (error | None, sha of the output)."""
    buf = ctypes.create_string_buffer(b"\xa5" * (cap + GUARD), cap + GUARD)
    used = ctypes.c_size_t(0)
    r = L.lz4f_mi355x_decompressFrame(buf, cap, frame, len(frame), ctypes.byref(used))
    assert buf.raw[cap:] == b"\xa5" * GUARD, "bytes behind the capacity were written"
    if L.LZ4F_isError(r):
        return L.LZ4F_getErrorName(r).decode(), None
    return None, sha(buf.raw[:r])


def stream_call(L, frame, seed=None):
    """LZ4F_decompress: whole (seed None: the whole frame per call, a block's room and more per call), or in 1..300-byte pieces
    with 1..500 bytes of room - the feed liblz4's pieces verdict was recorded with."""
    rng = np.random.default_rng(seed) if seed is not None else None
    d = ctypes.c_void_p(); L.LZ4F_createDecompressionContext(ctypes.byref(d), 100)
    out, pos = bytearray(), 0
    room = 512 if rng is not None else (8 << 20) + 64
    dst = ctypes.create_string_buffer(room)
    src = ctypes.create_string_buffer(frame, max(len(frame), 1))
    try:
        while True:
            sn, dn = (int(rng.integers(1, 301)), int(rng.integers(1, 501))) if rng is not None else (len(frame), room)
            ss, ds = ctypes.c_size_t(min(sn, len(frame) - pos)), ctypes.c_size_t(dn)
            r = L.LZ4F_decompress(d, dst, ctypes.byref(ds), ctypes.byref(src, pos), ctypes.byref(ss), None)
            if L.LZ4F_isError(r):
                return L.LZ4F_getErrorName(r).decode(), None
            out += dst.raw[:ds.value]; pos += ss.value
            if r == 0:
                return None, sha(bytes(out))
            if pos >= len(frame) and ds.value == 0:
                return "TRUNCATED", None
    finally:
        L.LZ4F_freeDecompressionContext(d)


SEEN = {}                        # switch set -> path bits seen (test_path_bits_seen)


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _self_indexed(name):
    return name.startswith(("end/sparse/full/bsid5/", "end/sparse/full/bsid7/"))


@pytest.mark.gpu
@pytest.mark.parametrize("ei", range(len(ENVS)), ids=["+".join(k[len("LZ4F_MI355X_"):] + ("=" + v if v != "1" else "") for k, v in e.items()) or "default" for e in ENVS])
def test_every_decoder_on_the_grammar_corpus(L, cases, ei):
    import collections
    import torch
    from lz4_frame_conduit_amd.device import Engine, DeviceCodecError
    env = ENVS[ei]
    seen, runs, bad = 0, 0, []

    def check(name, entry, want, err, got):
        nonlocal runs
        runs += 1
        if want is None and err is None:
            bad.append((name, entry, "accepted what liblz4 rejects"))
        elif want is not None and (err is not None or got != want):
            bad.append((name, entry, err or "other bytes"))

    os.environ.update(env)
    L.lz4f_mi355x_release_engines()
    try:
        eng = Engine(0)

        def dev_call(frame, cap):
            fr = torch.from_numpy(np.frombuffer(frame + bytes(32), dtype=np.uint8).copy()).cuda()
            back = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            try:
                eng.decompress_frame_async(fr, len(frame), back[:cap]); r = eng.result(); err = None
            except DeviceCodecError as e:
                r, err = None, str(e)
            torch.cuda.synchronize()
            assert bool((back[cap:] == 0xA5).all()), "bytes behind the capacity were written"
            return r, err, (None if err else sha(back[:r.size].cpu().numpy().tobytes()))

        def table_call(frame, meta, blocks):
            bs, n = meta["bs"], len(blocks)
            ent = np.zeros(n + 1, dtype=np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("word", "<u4"), ("dst_size", "<u4")]))
            for i, (p, w) in enumerate(blocks):
                ent[i] = (p, i * bs, w, bs)
            cap = max(n, 1) * bs
            back = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            fr = torch.from_numpy(np.frombuffer(frame + bytes(32), dtype=np.uint8).copy()).cuda()
            tb = torch.from_numpy(np.frombuffer(ent.tobytes(), dtype=np.uint8).copy()).cuda()
            info = _ffi.FrameInfo()
            info.blockSizeID, info.blockMode, info.blockChecksumFlag = (frame[5] >> 4) & 7, (frame[4] >> 5) & 1, (frame[4] >> 4) & 1
            try:
                eng.decompress_blocks_async(fr, len(frame), back[:cap], tb, n, info); r = eng.result(); err = None
            except DeviceCodecError as e:
                r, err = None, str(e)
            torch.cuda.synchronize()
            assert bool((back[cap:] == 0xA5).all()), "bytes behind the capacity were written"
            return r, err, (None if err else sha(back[:r.size].cpu().numpy().tobytes()))      # (short blocks are moved together)

        for ci, (name, frame, meta, want) in enumerate(cases):
            content, bs = meta["content"], meta["bs"]
            for cap in (content, content + 5, content + bs):
                err, got = host_call(L, frame, cap)
                check(name, "host@+%d" % (cap - content), want, err, got)
            blocks, end = _walk(frame)
            full_room = max(len(blocks), 1) * bs
            dcaps = [full_room] if meta["short_mid"] else sorted({content, content + 5, content + bs, full_room})
            for cap in dcaps:
                r, err, got = dev_call(frame, max(cap, 1))
                check(name, "device@+%d" % (cap - content), want, err, got)
                if r is not None:
                    seen |= int(r.flags) >> 12
                    if ei == 0 and _self_indexed(name) and ((int(r.flags) >> 12) & (PATH["self_index"] | DROPPED)) != PATH["self_index"]:
                        bad.append((name, "device@+%d" % (cap - content), "not self-indexed (path %#x)" % (int(r.flags) >> 12)))
            if end is not None:
                r, err, got = table_call(frame, meta, blocks)
                check(name, "table", want, err, got)
                if r is not None: seen |= int(r.flags) >> 12
            err, got = stream_call(L, frame)
            check(name, "stream", want, err, got)
            if len(frame) <= PIECES_MAX and (ei == 0 or ci % len(ENVS) == ei):
                err, got = stream_call(L, frame, zlib.crc32(name.encode()) if not name.startswith("hc/") else 7)
                check(name, "stream-pieces", want, err, got)
            try:
                got, err = sha(b"".join(conduit.decompressBatched([frame]))), None
            except Exception as e:                                          # (conduit.Lz4FrameError)
                got, err = None, str(e)
            check(name, "batched", want, err, got)
        eng.close()
    finally:
        for k in env: os.environ.pop(k, None)
        L.lz4f_mi355x_release_engines()
    SEEN[ei] = seen
    print("grammar corpus under %s: %d cases x entry points = %d decodes; path bits: %s"
          % (env or "{}", len(cases), runs, " ".join(sorted(k for k, v in PATH.items() if seen & v)) + (" walk_delivered" if seen & WALK_DELIVERED else "")))
    for (entry, err), n in sorted(collections.Counter((e.split("@")[0], x) for _, e, x in bad).items()):
        print("  disagreement: %-14s %-45s x%d" % (entry, err, n))
    for b in bad:
        print("   ", *b)
    assert not bad, (len(bad), bad[:20])


@pytest.mark.gpu
def test_path_bits_seen():
    """Over all switch sets (the tests above, run first), the corpus reached every decoder the path bits name."""
    assert sorted(SEEN) == list(range(len(ENVS))), "run the whole file: the switch-set tests record what they saw"
    seen = 0
    for v in SEEN.values(): seen |= v
    print("grammar corpus: path bits seen over %d switch sets: %s" % (len(ENVS), " ".join(sorted(k for k, v in PATH.items() if seen & v))))
    missing = [k for k, v in PATH.items() if not seen & v]
    assert not missing, ("path bits never seen", missing)
