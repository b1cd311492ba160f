"""Compression levels 3-12 (csrc/encode_hc.cuh): every compress entry point honours LZ4F_preferences_t.compressionLevel.

Sizes are held to liblz4's at the same level, as recorded in tests/golden/hc_sizes.json (tools/mint_hc_sizes.py); liblz4 itself is never
called here.  Every frame must decode byte-exact through the oracle and this library's decoders, and the bytes must be a function of
the input, its framing and the level alone, whichever entry point, engine, switch or device count made them.
Which bytes they are - the parse itself, match for match - is tests/test_gpu_hc_model.py's, against the model of tests/hc_model.py."""
import ctypes
import hashlib
import json
import lzma
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import golden_file
from lz4_frame_conduit_amd import _ffi, conduit, datagen
from lz4_frame_conduit_amd.device import Engine
from lz4_grammar import END_K
from lz4_writer_rules import audit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sha = lambda b: hashlib.sha256(b).hexdigest()
HC = json.loads(golden_file("hc_sizes.json"))
FRAMINGS = {name: dict(bsid=v[0], indep=v[1]) for name, v in HC["framings"].items()}
TOL = {"real_text": 1.03, "synth_text": 1.03, "synth50": 1.01}
ENGINES = {}


@pytest.fixture(scope="module")
def L():
    lib = _ffi.lib()
    assert lib.lz4f_mi355x_device_count() >= 1, "these tests need the MI355X"
    return lib


def real_text(n: int) -> bytes:
    text = lzma.decompress(golden_file("project_sources.txt.xz"))
    return (text * (n // len(text) + 1))[:n]


def hc_inputs():
    return {"real_text": real_text(HC["inputs"]["real_text"]), "synth_text": datagen.synth_text(HC["inputs"]["synth_text"]).tobytes(),
            "synth50": datagen.synth50(HC["inputs"]["synth50"]).tobytes()}


def prefs(level, bsid=4, indep=0, bck=0, cck=0, autoflush=0):
    return conduit.make_preferences(blockSizeID=bsid, blockMode=indep, blockChecksum=bck, contentChecksum=cck, autoFlush=autoflush,
                                    compressionLevel=level)


def engine(deterministic=False, fresh=False):
    if fresh:
        e = Engine(0)
        e.set_deterministic(deterministic)
        return e
    if deterministic not in ENGINES:
        ENGINES[deterministic] = Engine(0)
        ENGINES[deterministic].set_deterministic(deterministic)
    return ENGINES[deterministic]


def dev_compress(data: bytes, p, eng=None, inband=False) -> bytes:
    eng = eng or engine()
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    cap = eng.frame_bound_inband(len(data), p) if inband else eng.frame_bound(len(data), p)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    eng.compress_async(src, dst, p, inband=inband)
    r = eng.result()
    assert r.status == 0, r.status
    return dst[:r.size].cpu().numpy().tobytes()


def dev_decompress(frame: bytes, n: int, room: int = 0) -> bytes:
    """room: the output buffer's size when not n + 64 (a frame of short blocks: the device call bounds its walk by room / block size)."""
    eng = engine()
    src = torch.frombuffer(bytearray(frame), dtype=torch.uint8).cuda()
    dst = torch.zeros(max(room, n + 64), dtype=torch.uint8, device="cuda")
    eng.decompress_frame_async(src, len(frame), dst)
    r = eng.result()
    assert r.status == 0 and r.size == n, (r.status, r.size, n)
    return dst[:n].cpu().numpy().tobytes()


def bulk_compress(L, data: bytes, p) -> bytes:
    cap = L.lz4f_mi355x_compressFrameBound(len(data), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    r = L.lz4f_mi355x_compressFrame(dst, cap, data, len(data), ctypes.byref(p))
    assert not L.LZ4F_isError(r), (L.LZ4F_getErrorName(r), L.lz4f_mi355x_last_error())
    return dst.raw[:r]


def bulk_decompress(L, frame: bytes, n: int) -> bytes:
    dst = ctypes.create_string_buffer(n + 8)
    used = ctypes.c_size_t(0)
    r = L.lz4f_mi355x_decompressFrame(dst, n + 8, frame, len(frame), ctypes.byref(used))
    assert not L.LZ4F_isError(r), (L.LZ4F_getErrorName(r), L.lz4f_mi355x_last_error())
    assert used.value == len(frame)
    return dst.raw[:r]


def stream_compress(L, data: bytes, p, rng, max_slice=3 << 20) -> bytes:
    """LZ4F_compressBegin / Update (random slice sizes, no flush) / End."""
    c = ctypes.c_void_p()
    assert L.LZ4F_createCompressionContext(ctypes.byref(c), 100) == 0
    hdr = ctypes.create_string_buffer(32)
    r = L.LZ4F_compressBegin(c, hdr, 32, ctypes.byref(p))
    assert not L.LZ4F_isError(r), L.LZ4F_getErrorName(r)
    out = [hdr.raw[:r]]
    pos = 0
    while pos < len(data):
        k = min(int(rng.integers(1, max_slice)), len(data) - pos)
        bound = L.LZ4F_compressBound(k, ctypes.byref(p))
        dst = ctypes.create_string_buffer(bound)
        r = L.LZ4F_compressUpdate(c, dst, bound, data[pos:pos + k], k, None)
        assert not L.LZ4F_isError(r), (L.LZ4F_getErrorName(r), L.lz4f_mi355x_last_error())
        out.append(dst.raw[:r])
        pos += k
    eb = L.LZ4F_compressBound(0, ctypes.byref(p))
    ed = ctypes.create_string_buffer(eb)
    r = L.LZ4F_compressEnd(c, ed, eb, None)
    assert not L.LZ4F_isError(r)
    out.append(ed.raw[:r])
    L.LZ4F_freeCompressionContext(c)
    return b"".join(out)


def stream_decompress(frame: bytes) -> bytes:
    return b"".join(conduit.decompress(conduit.bsChunksOf(100003, frame)))


def oracle_ok(frame: bytes, data: bytes):
    out, used = oracle.decompress_frame(frame, cap=len(data) + 64)
    assert used == len(frame) and out == data


# ------------------------------------------------------------------------------------------------
def test_hc_sizes_against_liblz4(L):
    """Every input, framing and level of hc_sizes.json through dev_compressFrame: the oracle and the device decoder give the input back,
    and the frame is within TOL of liblz4's frame at the same level."""
    worst = {}
    for name, data in hc_inputs().items():
        for fr, kw in FRAMINGS.items():
            for lvl in HC["levels"]:
                frame = dev_compress(data, prefs(lvl, **kw))
                oracle_ok(frame, data)
                assert dev_decompress(frame, len(data)) == data, (name, fr, lvl)
                ref = HC["sizes"]["%s/%s/%d" % (name, fr, lvl)]
                worst[(name, fr, lvl)] = len(frame) / ref
                assert len(frame) <= ref * TOL[name], (name, fr, lvl, len(frame), ref, len(frame) / ref)
    print("size / liblz4's, worst per input:", {n: max(v for k, v in worst.items() if k[0] == n) for n in TOL})


def test_levels_are_ordered(L):
    """Real text: a higher level never gives a bigger frame, level 3 is well below level 0's frame, levels beyond 12 are 12, and with
    the deterministic switch on every level <= 2 (negative ones included) is the fast encoder's level 0."""
    data = real_text(8 << 20)
    for fr, kw in FRAMINGS.items():
        sizes = [len(dev_compress(data, prefs(lvl, **kw))) for lvl in (3, 6, 9, 12)]
        assert sizes == sorted(sizes, reverse=True), (fr, sizes)
        lvl0 = dev_compress(data, prefs(0, **kw), eng=engine(True))
        assert sizes[0] <= 0.80 * len(lvl0), (fr, sizes[0], len(lvl0))
        twelve = dev_compress(data, prefs(12, **kw))
        for lvl in (13, 100):
            assert dev_compress(data, prefs(lvl, **kw)) == twelve, (fr, lvl)
        for lvl in (-1, 1, 2):
            assert dev_compress(data, prefs(lvl, **kw), eng=engine(True)) == lvl0, (fr, lvl)


_BULK_CHILD = r"""
import ctypes, hashlib, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from lz4_frame_conduit_amd import _ffi, conduit
from test_gpu_hc import real_text, prefs, bulk_compress
L = _ffi.lib()
data = real_text(%d)
for devs in (1, 2):
    assert L.lz4f_mi355x_use_devices(devs) == 0
    for lvl, bsid, indep in %r:
        print(devs, lvl, bsid, indep, hashlib.sha256(bulk_compress(L, data, prefs(lvl, bsid, indep))).hexdigest())
L.lz4f_mi355x_use_devices(1)
print("ok")
"""


def test_deterministic_by_construction(L):
    """Levels 3 and 12, 64 KiB independent and linked blocks, an input longer than a bulk slab (64 MiB): the same frame from two runs,
    two engines, the deterministic switch on and off, dev_compressFrame, the in-band indexed call without its trailer, the host bulk
    call over 1 and 2 logical devices, and streaming with random slices."""
    n = (64 << 20) + (5 << 20) + 12345
    data = real_text(n)
    rng = np.random.default_rng(3)
    cases = [(lvl, 4, indep) for lvl in (3, 12) for indep in (1, 0)]
    want = {}
    for lvl, bsid, indep in cases:
        p = prefs(lvl, bsid, indep)
        a = dev_compress(data, p)
        assert dev_compress(data, p) == a
        for det in (False, True):
            e = engine(det, fresh=True)
            assert dev_compress(data, p, eng=e) == a, (lvl, indep, det)
            e.close()
        inb = dev_compress(data, p, inband=True)
        assert inb[:len(a)] == a and len(inb) > len(a), (lvl, indep)
        assert 0x184D2A50 <= int.from_bytes(inb[len(a):len(a) + 4], "little") <= 0x184D2A5F
        assert bulk_compress(L, data, p) == a, (lvl, indep)
        assert stream_compress(L, data, p, rng, max_slice=12 << 20) == a, (lvl, indep)
        oracle_ok(a, data)
        want[(lvl, bsid, indep)] = sha(a)
    code = _BULK_CHILD % (ROOT, os.path.join(ROOT, "tests"), n, cases)
    env = dict(os.environ)
    env["LZ4F_MI355X_LOGICAL_DEVICES"] = "2"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    for line in r.stdout.strip().splitlines()[:-1]:
        devs, lvl, bsid, indep, h = line.split()
        assert h == want[(int(lvl), int(bsid), int(indep))], line


def test_every_surface_decodes(L, tmp_path):
    """HC frames from every compress surface decode byte-exact through the oracle and this library's streaming, bulk and device
    decoders, with and without the block-list trailer."""
    data = real_text(3 << 20) + datagen.synth50(1 << 20, 5).tobytes() + b"tail" * 1000
    rng = np.random.default_rng(9)

    def check(frame, with_trailer=False, room=0):
        out, used = oracle.decompress_frame(frame, cap=len(data) + 64)
        assert out == data
        lz, rest = frame[:used], frame[used:]
        assert bool(rest) == with_trailer
        if rest:
            assert 0x184D2A50 <= int.from_bytes(rest[:4], "little") <= 0x184D2A5F
        listed = frame if rest else conduit.appendBlockList(lz)
        assert stream_decompress(lz) == data
        assert bulk_decompress(L, lz, len(data)) == data
        for f in (lz, listed):
            assert dev_decompress(f, len(data), room) == data
            assert b"".join(conduit.decompressBatched([f])) == data

    for lvl in (3, 9, 12):
        for kw in (dict(bsid=4, indep=0), dict(bsid=5, indep=1, bck=1, cck=1), dict(bsid=7, indep=0, bck=1)):
            p = prefs(lvl, **kw)
            check(b"".join(conduit.compressWithPreferences(p, conduit.bsChunksOf(77777, data))))
            check(b"".join(conduit.compressBatched(conduit.bsChunksOf(500001, data), p, batchBytes=1 << 20)))
            check(b"".join(conduit.compressBatched(conduit.bsChunksOf(500001, data), p, batchBytes=1 << 20, blockList=True)), True)
            pa = prefs(lvl, autoflush=1, **kw)
            check(stream_compress(L, data, pa, rng, max_slice=200000), room=len(data) + ((len(data) // 50000 + 8) << (16 + 2 * (kw["bsid"] - 4))))
            check(dev_compress(data, p, inband=True), True)
    cli = os.path.join(ROOT, "lz4_frame_conduit_amd", "mi355x-lz4c")
    src, dst = tmp_path / "in.bin", tmp_path / "out.lz4"
    src.write_bytes(data)
    for flag in ("-9", "--best", "-3"):
        r = subprocess.run([cli, flag, str(src), str(dst)], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        frame = dst.read_bytes()
        oracle_ok(frame, data)
        lvl = 12 if flag == "--best" else int(flag[1:])
        assert len(frame) < len(b"".join(conduit.compressBatched([data], prefs(0)))) * 0.85, flag
        assert frame == b"".join(conduit.compressBatched([data], prefs(lvl))), flag


def _edge_inputs():
    rng = np.random.default_rng(77)
    text = real_text(1 << 20)
    out = {}
    for n in range(0, 33):
        out["short%d" % n] = (b"abcab" * 8)[:n]
    for k in END_K:                                         # a repeat that ends k bytes before a block / chunk end
        for end in (65536, 131072):
            out["end%d_k%d" % (end, k)] = text[:end - k - 200] + text[1000:1200] + bytes(rng.integers(0, 256, k, dtype=np.uint8))
    out["zeros8m"] = bytes(8 << 20)
    for d in (1, 2, 3):
        out["period%d" % d] = (bytes(rng.integers(0, 256, d, dtype=np.uint8)) * ((300000 // d) + 1))[:300000]
    out["random"] = bytes(rng.integers(0, 256, 5 << 20, dtype=np.uint8))
    far = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    # a 1000-byte repeat exactly 65535 back (big enough to pay for the 64 KiB literal run's 261 length bytes), and one byte too far
    out["far65535"] = far[:1000] + far[1000:65535 + 1000] + far[1000:2000] + far[:64]
    out["far65536"] = far[:1000] + far[1000:65536 + 1000] + far[1000:2000] + far[:64]
    b1, b2 = bytes(rng.integers(0, 256, 65536, dtype=np.uint8)), bytes(rng.integers(0, 256, 65536, dtype=np.uint8))
    out["linked_deep"] = b1 + b2 + b2[1:4001] + bytes(rng.integers(0, 256, 1000, dtype=np.uint8))   # block 3 opens with a match 65535 back
    return out


def test_grammar_edges(L):
    """Inputs at the LZ4 block grammar's edges at levels 3 and 12: each frame round-trips through the oracle (and through the device
    decoder) and breaks no writer rule (lz4_writer_rules.audit), in 64 KiB and 4 MiB blocks, independent and linked."""
    for name, data in _edge_inputs().items():
        for lvl in (3, 12):
            for kw in (dict(bsid=4, indep=1), dict(bsid=4, indep=0), dict(bsid=7, indep=1)):
                frame = dev_compress(data, prefs(lvl, **kw))
                oracle_ok(frame, data)
                assert audit(frame, data, dict(bsid=kw["bsid"], linked=not kw["indep"], bck=False, cck=False)) == [], (name, lvl, kw)
                if data:
                    assert dev_decompress(frame, len(data)) == data, (name, lvl, kw)
                if name == "random":
                    assert len(frame) <= len(data) + 64 * ((len(data) >> 16) + 1), (name, len(frame))        # stored blocks
                if name == "zeros8m":
                    assert len(frame) < len(data) // 200, (name, kw, len(frame))
                if name == "far65535" and kw["bsid"] == 7:
                    assert len(frame) < len(data) - 500, (name, len(frame))
                if name == "linked_deep" and kw == dict(bsid=4, indep=0):
                    assert len(frame) < len(data) - 3500, (name, len(frame))
