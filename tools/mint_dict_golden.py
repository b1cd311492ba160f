#!/usr/bin/env python3
"""Mint tests/golden/dict_frames.json: liblz4's frames and verdicts for the shared-dictionary cases of tests/dict_cases.py.

Run on a machine that has liblz4 (>= 1.9.0: LZ4F_createCDict, LZ4F_compressFrame_usingCDict, LZ4F_decompress_usingDict); the
tests never need it.  For every dictionary (64 KiB blocks):
  natural   each record compressed with LZ4F_compressFrame_usingCDict as an independent frame - and as a linked one too where it
            is longer than a block (liblz4 writes a single block as an independent one whatever was asked for); the frame is stored,
            decoded back with LZ4F_decompress_usingDict as a check, and - records of at most 4096 bytes - also compressed without
            a dictionary: the two totals are what the ratio tests compare the device's total to;
  planted   each hand-built frame given to LZ4F_decompress_usingDict block by block: accepted (the output's length and SHA-256) or
            rejected (the block at which liblz4 said so).
Inputs, dictionaries and planted frames are stored as SHA-256 only: tests/dict_cases.py rebuilds them.

    python tools/mint_dict_golden.py [path to liblz4.so]
"""
import base64
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dict_cases as dc      # noqa: E402
import oracle                # noqa: E402

vp, sz = ctypes.c_void_p, ctypes.c_size_t


def liblz4(path):
    L = ctypes.CDLL(path)
    for name, res, args in (("LZ4F_createCDict", vp, [vp, sz]), ("LZ4F_freeCDict", None, [vp]),
                            ("LZ4F_createCompressionContext", sz, [ctypes.POINTER(vp), ctypes.c_uint]), ("LZ4F_freeCompressionContext", sz, [vp]),
                            ("LZ4F_compressFrameBound", sz, [sz, vp]),
                            ("LZ4F_compressFrame_usingCDict", sz, [vp, vp, sz, vp, sz, vp, vp]),
                            ("LZ4F_createDecompressionContext", sz, [ctypes.POINTER(vp), ctypes.c_uint]), ("LZ4F_freeDecompressionContext", sz, [vp]),
                            ("LZ4F_decompress_usingDict", sz, [vp, vp, ctypes.POINTER(sz), vp, ctypes.POINTER(sz), vp, sz, vp]),
                            ("LZ4F_isError", ctypes.c_uint, [sz]), ("LZ4_versionString", ctypes.c_char_p, [])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def compress(L, data: bytes, d: bytes, indep: bool) -> bytes:
    """LZ4F_compressFrame_usingCDict (d empty: no dictionary), 64 KiB blocks, level 0."""
    prefs = oracle.mkprefs(bsid=4, indep=1 if indep else 0)
    cctx = vp()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(cctx), 100))
    cdict = L.LZ4F_createCDict(d, len(d)) if d else None
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(prefs))
    out = ctypes.create_string_buffer(cap)
    r = L.LZ4F_compressFrame_usingCDict(cctx, out, cap, data, len(data), cdict, ctypes.byref(prefs))
    assert not L.LZ4F_isError(r)
    if cdict: L.LZ4F_freeCDict(cdict)
    L.LZ4F_freeCompressionContext(cctx)
    return out.raw[:r]


def decompress(L, frame: bytes, d: bytes):
    """LZ4F_decompress_usingDict, the frame fed header first and then block by block -> (output, None), or (None, the block
    liblz4 rejected it at; -1: outside the blocks)."""
    f = dc.walk(frame)
    cuts = [f["blocks"][0][1] - 4 if f["blocks"] else len(frame)]
    for k, (_, at, n) in enumerate(f["blocks"]):
        cuts.append(f["blocks"][k + 1][1] - 4 if k + 1 < len(f["blocks"]) else at + n + (4 if f["bck"] else 0))
    cuts.append(len(frame))
    dctx = vp()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(dctx), 100))
    out, pos, verdict = bytearray(), 0, None
    buf = ctypes.create_string_buffer(1 << 20)
    try:
        for k, cut in enumerate(cuts):
            while pos < cut:
                dn, sn = sz(len(buf)), sz(cut - pos)
                r = L.LZ4F_decompress_usingDict(dctx, buf, ctypes.byref(dn), frame[pos:cut], ctypes.byref(sn), d, len(d), None)
                if L.LZ4F_isError(r):
                    verdict = k - 1 if 1 <= k <= len(f["blocks"]) else -1
                    return None, verdict
                out += buf.raw[:dn.value]
                pos += sn.value
                assert sn.value or dn.value
        assert r == 0, "frame not complete"
        return bytes(out), None
    finally:
        L.LZ4F_freeDecompressionContext(dctx)


def main():
    L = liblz4(sys.argv[1] if len(sys.argv) > 1 else "liblz4.so.1")
    fx = {"liblz4": L.LZ4_versionString().decode(), "dicts": {}, "natural": [], "planted": [], "totals": {}}
    for dname in dc.DICT_LEN:
        d = dc.dictionary(dname)
        fx["dicts"][dname] = {"len": len(d), "sha256": dc.sha(d)}
        fx["totals"][dname] = {}
        for mode in dc.MODES:
            tot = {"with": 0, "without": 0, "records": 0}
            for name, data in dc.natural(dname):
                if mode == "linked" and len(data) <= dc.KB64:
                    continue                                          # (liblz4 writes a single block as an independent one whatever was asked for)
                frame = compress(L, data, d, mode == "indep")
                got, bad = decompress(L, frame, d)
                assert got == data, (dname, mode, name, bad)
                assert dc.model_decode(frame, d).out == data, ("the model does not decode liblz4's frame", dname, mode, name)
                fx["natural"].append({"dict": dname, "mode": mode, "name": name, "len": len(data), "sha256": dc.sha(data),
                                      "frame": base64.b64encode(frame).decode()})
                if len(data) <= dc.RATIO_MAX:
                    tot["with"] += len(frame); tot["without"] += len(compress(L, data, b"", mode == "indep")); tot["records"] += 1
            if mode == "indep": fx["totals"][dname] = tot
        for name, mode, frame in dc.planted(dname):
            got, bad = decompress(L, frame, d)
            e = {"dict": dname, "mode": mode, "name": name, "sha256": dc.sha(frame), "ok": got is not None, "bad_block": bad}
            if got is not None: e["out_len"], e["out_sha256"] = len(got), dc.sha(got)
            fx["planted"].append(e)
    with open(dc.FIXTURE, "w") as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write("\n")
    n_ok = sum(e["ok"] for e in fx["planted"])
    print("%s: %d natural frames, %d planted (%d accepted, %d rejected), %d bytes; liblz4 %s" % (
        os.path.relpath(dc.FIXTURE, ROOT), len(fx["natural"]), len(fx["planted"]), n_ok, len(fx["planted"]) - n_ok, os.path.getsize(dc.FIXTURE), fx["liblz4"]))
    for dname, t in fx["totals"].items():
        print("  %-7s" % dname, t, round(t["without"] / max(t["with"], 1), 2))


if __name__ == "__main__":
    main()
