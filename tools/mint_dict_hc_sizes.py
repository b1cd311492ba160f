#!/usr/bin/env python3
"""Mint tests/golden/dict_hc_sizes.json: what liblz4 makes of the ratio corpus of tests/dict_cases.py with a dictionary, level by level.

Host only.  Run on a machine that has liblz4 (>= 1.9.0: LZ4F_createCDict, LZ4F_compressFrame_usingCDict); the tests never need it.
The corpus: the phrase dictionary's natural records of at most 4096 bytes, each an independent frame of 64 KiB blocks.  For the
levels 0, 3, 6, 9 and 12 the fixture holds liblz4's total with the CDict and without a dictionary - the yardstick of the prepared
dictionary's hash-chain digest (tests/test_gpu_cdict_hc.py) - and the SHA-256 of the dictionary and of every input: sizes and hashes
only, no frames.

    python tools/mint_dict_hc_sizes.py [path to liblz4.so]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dict_cases as dc      # noqa: E402
import oracle                # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "dict_hc_sizes.json")
DNAME = "phrase"
LEVELS = (0, 3, 6, 9, 12)
vp, sz = ctypes.c_void_p, ctypes.c_size_t


def liblz4(path):
    L = ctypes.CDLL(path)
    for name, res, args in (("LZ4F_createCDict", vp, [vp, sz]), ("LZ4F_freeCDict", None, [vp]),
                            ("LZ4F_createCompressionContext", sz, [ctypes.POINTER(vp), ctypes.c_uint]), ("LZ4F_freeCompressionContext", sz, [vp]),
                            ("LZ4F_compressFrameBound", sz, [sz, vp]),
                            ("LZ4F_compressFrame_usingCDict", sz, [vp, vp, sz, vp, sz, vp, vp]),
                            ("LZ4F_isError", ctypes.c_uint, [sz]), ("LZ4_versionString", ctypes.c_char_p, [])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def frame_size(L, cctx, data: bytes, cdict, level: int) -> int:
    """The bytes of LZ4F_compressFrame_usingCDict's frame (cdict None: no dictionary): independent 64 KiB blocks."""
    prefs = oracle.mkprefs(bsid=4, indep=1)
    prefs.compressionLevel = level
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(prefs))
    out = ctypes.create_string_buffer(cap)
    r = L.LZ4F_compressFrame_usingCDict(cctx, out, cap, data, len(data), cdict, ctypes.byref(prefs))
    assert not L.LZ4F_isError(r)
    return int(r)


def corpus():
    return [(name, data) for name, data in dc.natural(DNAME) if len(data) <= dc.RATIO_MAX]


def main():
    L = liblz4(sys.argv[1] if len(sys.argv) > 1 else "liblz4.so.1")
    d = dc.dictionary(DNAME)
    recs = corpus()
    fx = {"liblz4": L.LZ4_versionString().decode(), "dict": {"name": DNAME, "len": len(d), "sha256": dc.sha(d)},
          "inputs": [{"name": name, "len": len(data), "sha256": dc.sha(data)} for name, data in recs],
          "records": len(recs), "bytes": sum(len(data) for _, data in recs), "totals": {}}
    cctx = vp()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(cctx), 100))
    cdict = L.LZ4F_createCDict(d, len(d))
    assert cdict
    for level in LEVELS:
        fx["totals"][str(level)] = {"with": sum(frame_size(L, cctx, data, cdict, level) for _, data in recs),
                                    "without": sum(frame_size(L, cctx, data, None, level) for _, data in recs)}
    L.LZ4F_freeCDict(cdict)
    L.LZ4F_freeCompressionContext(cctx)
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d records, %d bytes; liblz4 %s" % (os.path.relpath(FIXTURE, ROOT), fx["records"], fx["bytes"], fx["liblz4"]))
    for level in LEVELS:
        print("  level %-2d" % level, fx["totals"][str(level)])


if __name__ == "__main__":
    main()
