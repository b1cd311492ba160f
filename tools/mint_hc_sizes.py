"""Record liblz4's frame sizes at the high-compression levels: tests/golden/hc_sizes.json.

Drives the system liblz4 (liblz4.so.1) through ctypes with LZ4F_compressFrame at levels 3, 6, 9 and 12 over three inputs - 24 MiB of
real text (built as tests/test_gpu_parity.py's _real_text builds it), 8 MiB of datagen.synth_text and 8 MiB of datagen.synth50 - in
4 MiB independent, 64 KiB independent and 64 KiB linked blocks.  The GPU tests read only the JSON (tests/test_gpu_hc.py): they never
call liblz4.  Host only; run from the repository root:  python tools/mint_hc_sizes.py
"""
import ctypes
import json
import lzma
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lz4_frame_conduit_amd import datagen  # noqa: E402

LEVELS = (3, 6, 9, 12)
FRAMINGS = {"indep4m": (7, 1), "indep64k": (4, 1), "linked64k": (4, 0)}     # name -> (blockSizeID, blockMode: 0 linked, 1 independent)


def real_text(n: int) -> bytes:
    text = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "project_sources.txt.xz"), "rb").read())
    return (text * (n // len(text) + 1))[:n]


def inputs():
    return {
        "real_text": real_text(24 << 20),
        "synth_text": datagen.synth_text(8 << 20).tobytes(),
        "synth50": datagen.synth50(8 << 20).tobytes(),
    }


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Prefs(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def main():
    lz = ctypes.CDLL("liblz4.so.1")
    lz.LZ4F_compressFrameBound.restype = ctypes.c_size_t
    lz.LZ4F_compressFrame.restype = ctypes.c_size_t
    lz.LZ4F_isError.restype = ctypes.c_uint
    out = {"liblz4_version": lz.LZ4_versionNumber(), "levels": list(LEVELS), "framings": {k: list(v) for k, v in FRAMINGS.items()},
           "inputs": {}, "sizes": {}}
    for name, data in inputs().items():
        out["inputs"][name] = len(data)
        for fr, (bsid, mode) in FRAMINGS.items():
            for lvl in LEVELS:
                p = Prefs()
                p.frameInfo.blockSizeID, p.frameInfo.blockMode, p.compressionLevel = bsid, mode, lvl
                cap = lz.LZ4F_compressFrameBound(ctypes.c_size_t(len(data)), ctypes.byref(p))
                buf = ctypes.create_string_buffer(cap)
                r = lz.LZ4F_compressFrame(buf, ctypes.c_size_t(cap), data, ctypes.c_size_t(len(data)), ctypes.byref(p))
                assert not lz.LZ4F_isError(ctypes.c_size_t(r)), (name, fr, lvl)
                out["sizes"]["%s/%s/%d" % (name, fr, lvl)] = r
                print(name, fr, lvl, r, "%.3f" % (len(data) / r), flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "hc_sizes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
