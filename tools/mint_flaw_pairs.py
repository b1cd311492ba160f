#!/usr/bin/env python3
"""Mint tests/golden/flaw_pairs.json: liblz4's answer to every two-flaw frame of tests/flaw_pairs.py, and to each flaw alone.

Run on a machine that has liblz4; no test needs it.  Every frame goes through LZ4F_decompress twice: whole (the whole frame and
all the room per call) and in pieces (1..300 bytes of input and 1..500 bytes of room per call, seeded by the case's name - the feed
tests/test_gpu_flaw_pairs.py repeats).  A room@b case gets that much room in all, and no more.  Recorded per feed:
  error        liblz4's error name, or null
  stall        "input" / "room": liblz4 reported no error and stopped making progress - its answer to a truncated frame and to a
               window that ends inside a block - or null
  out_sha256   the output's SHA-256 when the frame was decoded to its end, else null
and per case the frame's SHA-256: tests/flaw_pairs.py rebuilds the frames from their names.  Names and hashes only.

    python tools/mint_flaw_pairs.py [path to liblz4.so]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import flaw_pairs as fp      # noqa: E402

vp, sz = ctypes.c_void_p, ctypes.c_size_t


def liblz4(path):
    L = ctypes.CDLL(path)
    for name, res, args in (("LZ4F_createDecompressionContext", sz, [ctypes.POINTER(vp), ctypes.c_uint]), ("LZ4F_freeDecompressionContext", sz, [vp]),
                            ("LZ4F_decompress", sz, [vp, vp, ctypes.POINTER(sz), vp, ctypes.POINTER(sz), vp]),
                            ("LZ4F_isError", ctypes.c_uint, [sz]), ("LZ4F_getErrorName", ctypes.c_char_p, [sz]), ("LZ4_versionString", ctypes.c_char_p, [])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def main():
    L = liblz4(sys.argv[1] if len(sys.argv) > 1 else "liblz4.so.1")
    fx = {"liblz4": L.LZ4_versionString().decode(), "cases": {}}
    for c in fp.cases():
        budget = fp.room_window(c, False) if c.room is not None else fp.ample(c)
        fx["cases"][c.name] = {"frame_sha256": fp.sha(c.frame), "once": fp.feed(L, c.frame, budget),
                               "pieces": fp.feed(L, c.frame, budget, fp.pieces_seed(c))}
    with open(fp.FIXTURE, "w") as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write("\n")
    words = [fp.ref_verdict(r["once"]).split(":")[0] for r in fx["cases"].values()]
    print("%s: %d cases, %d bytes; liblz4 %s" % (os.path.relpath(fp.FIXTURE, ROOT), len(fx["cases"]), os.path.getsize(fp.FIXTURE), fx["liblz4"]))
    for w in sorted(set(words)):
        print("  %-36s %d" % (w, words.count(w)))
    differ = sum(fp.ref_verdict(r["once"]) != fp.ref_verdict(r["pieces"]) for r in fx["cases"].values())
    print("  whole and pieces differ (beyond the two names of a failed block): %d" % differ)


if __name__ == "__main__":
    main()
