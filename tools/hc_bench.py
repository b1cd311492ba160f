"""Compression levels 3-12 on device-resident input: milliseconds, GiB/s and ratio per input, framing and level, beside liblz4 at the
same level on 16 host threads (where the system's liblz4.so.1 loads; each thread compresses its share of the blocks as frames of their own).

    python tools/hc_bench.py [--gib 1] [--levels 3,6,9,12] [--reps 2] [--no-liblz4]

Inputs: real text (this project's sources, tests/golden/project_sources.txt.xz, repeated), datagen.synth_text (Zipf text) and
datagen.synth50; framings: 4 MiB and 64 KiB independent blocks.  The GPU figure is the best of --reps timed calls after a warm-up,
compress_async + result (the frame stays in HBM).  Prints one line per case and a JSON summary line at the end.
"""
import argparse
import ctypes
import json
import lzma
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lz4_frame_conduit_amd import conduit, datagen  # noqa: E402
from lz4_frame_conduit_amd.device import Engine  # noqa: E402

FRAMINGS = {"indep4m": 7, "indep64k": 4}


def real_text(n: int) -> np.ndarray:
    text = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "project_sources.txt.xz"), "rb").read())
    return np.frombuffer((text * (n // len(text) + 1))[:n], dtype=np.uint8)


class _FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int), ("frameType", ctypes.c_int),
                ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint), ("blockChecksumFlag", ctypes.c_int)]


class _Prefs(ctypes.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint), ("favorDecSpeed", ctypes.c_uint),
                ("reserved", ctypes.c_uint * 3)]


def liblz4_time(lz, data: np.ndarray, bsid: int, level: int, threads: int = 16):
    """Seconds and bytes for liblz4 LZ4F_compressFrame at `level`, the input cut into `threads` runs of whole blocks."""
    bs = {4: 64 << 10, 7: 4 << 20}[bsid]
    nblk = (len(data) + bs - 1) // bs
    per = (nblk + threads - 1) // threads
    parts = [data[i * per * bs:(i + 1) * per * bs] for i in range(threads)]
    parts = [p for p in parts if len(p)]
    p = _Prefs()
    p.frameInfo.blockSizeID, p.frameInfo.blockMode, p.compressionLevel = bsid, 1, level

    def one(part):
        cap = lz.LZ4F_compressFrameBound(ctypes.c_size_t(len(part)), ctypes.byref(p))
        buf = ctypes.create_string_buffer(cap)
        return lz.LZ4F_compressFrame(buf, ctypes.c_size_t(cap), part.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(part)), ctypes.byref(p))

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        sizes = list(ex.map(one, parts))
        return time.perf_counter() - t0, sum(sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--levels", default="3,6,9,12")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-liblz4", action="store_true")
    a = ap.parse_args()
    n = int(a.gib * (1 << 30)) // (1 << 20) << 20
    levels = [int(x) for x in a.levels.split(",")]
    lz = None
    if not a.no_liblz4:
        try:
            lz = ctypes.CDLL("liblz4.so.1")
            lz.LZ4F_compressFrameBound.restype = ctypes.c_size_t
            lz.LZ4F_compressFrame.restype = ctypes.c_size_t
        except OSError:
            lz = None
    eng = Engine(0)
    rows = []
    for name, make in (("real_text", real_text), ("synth_text", lambda k: datagen.synth_text(k)), ("synth50", lambda k: datagen.synth50(k))):
        host = make(n)
        src = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        for fr, bsid in FRAMINGS.items():
            for lvl in levels:
                p = conduit.make_preferences(blockSizeID=bsid, blockMode=1, compressionLevel=lvl)
                dst = torch.empty(eng.frame_bound(n, p), dtype=torch.uint8, device="cuda")
                eng.compress_async(src, dst, p)
                r = eng.result()
                best = None
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eng.compress_async(src, dst, p)
                    r = eng.result()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                row = dict(input=name, framing=fr, level=lvl, ms=round(best * 1e3, 2), gib_s=round(n / best / (1 << 30), 3), ratio=round(n / r.size, 4))
                if lz is not None:
                    t, size = liblz4_time(lz, host, bsid, lvl)
                    row.update(liblz4_ms=round(t * 1e3, 1), liblz4_gib_s=round(n / t / (1 << 30), 3), liblz4_ratio=round(n / size, 4),
                               speedup=round(t / best, 1))
                rows.append(row)
                print(" ".join("%s=%s" % kv for kv in row.items()), flush=True)
        del src
    eng.close()
    print(json.dumps({"hc_bench": rows, "bytes": n}))


if __name__ == "__main__":
    main()
