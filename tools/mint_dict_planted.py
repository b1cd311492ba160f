#!/usr/bin/env python3
"""Mint tests/golden/dict_planted.json: what liblz4 writes of the planted dictionary cases of tests/dict_encoder_cases.py.

Host only.  Run on a machine that has liblz4 (>= 1.9.0: LZ4F_createCDict, LZ4F_compressFrame_usingCDict); the tests never need it.
For every case and each of its framings the input goes through LZ4F_compressFrame_usingCDict with the case's dictionary at levels
0 and 9, the frame is decoded back by the dictionary model as a check, and the fixture keeps
  - the SHA-256 of every dictionary and of every input (tests/dict_encoder_cases.py rebuilds both),
  - the frame's size at both levels,
  - the frame's raw sequences per block at both levels as [literals, match length, offset] (null: a stored block):
no frames, no bytes of any input.  A (case, framing) whose level-9 sequences are the planted parse is `forced`
(dict_encoder_cases.is_forced): what the hash-chain encoders of the device are held to.

    python tools/mint_dict_planted.py [path to liblz4.so]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dict_cases as dc               # noqa: E402
import dict_encoder_cases as de       # noqa: E402
import encoder_cases as ec            # noqa: E402
import oracle                         # noqa: E402

LEVELS = (0, 9)
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


def compress(L, cctx, data: bytes, cdict, fr: str, level: int) -> bytes:
    f = ec.FRAMINGS[fr]
    prefs = oracle.mkprefs(bsid=f["bsid"], indep=0 if f["linked"] else 1, bck=int(f["bck"]), cck=int(f["cck"]))
    prefs.compressionLevel = level
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(prefs))
    out = ctypes.create_string_buffer(cap)
    r = L.LZ4F_compressFrame_usingCDict(cctx, out, cap, data, len(data), cdict, ctypes.byref(prefs))
    assert not L.LZ4F_isError(r)
    return out.raw[:r]


def main():
    L = liblz4(sys.argv[1] if len(sys.argv) > 1 else "liblz4.so.1")
    cctx = vp()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(cctx), 100))
    dicts, cases = {}, {}
    for dname in de.DICT_LEN:
        d = de.dictionary(dname)
        dicts[dname] = {"len": len(d), "sha256": dc.sha(d)}
        cdict = L.LZ4F_createCDict(d, len(d))
        assert cdict
        for c in de.corpus():
            if c.dname != dname: continue
            data = c.data
            e = {"dict": dname, "len": len(data), "sha256": dc.sha(data)}
            for fr in c.framings:
                e[fr] = {}
                for level in LEVELS:
                    frame = compress(L, cctx, data, cdict, fr, level)
                    v = dc.model_decode(frame, d)
                    assert v.ok and v.out == data and v.consumed == len(frame), (c.name, fr, level, v.why)
                    e[fr]["size%d" % level] = len(frame)
                    e[fr]["seqs%d" % level] = [None if S is None else [list(s) for s in S] for S in de.frame_seqs(frame)]
            cases[c.name] = e
        L.LZ4F_freeCDict(cdict)
    L.LZ4F_freeCompressionContext(cctx)
    fx = {"liblz4": L.LZ4_versionString().decode(), "dicts": dicts, "cases": cases}
    lines = ['"liblz4": %s,' % json.dumps(fx["liblz4"]), '"dicts": %s,' % json.dumps(dicts, sort_keys=True, separators=(",", ":")), '"cases": {']
    lines += ["%s: %s%s" % (json.dumps(n), json.dumps(cases[n], sort_keys=True, separators=(",", ":")), "," if k + 1 < len(cases) else "")
              for k, n in enumerate(sorted(cases))]
    with open(de.FIXTURE, "w") as f:
        f.write("{\n" + "\n".join(lines) + "\n}}\n")
    fx = de.load_fixture()
    pairs = de.pairs()
    forced = [(c, fr) for c, fr in pairs if de.is_forced(fx, c, fr)]
    print("%s: %d cases, %d (case, framing) pairs, %d forced, %d bytes; liblz4 %s" % (
        os.path.relpath(de.FIXTURE, ROOT), len(cases), len(pairs), len(forced), os.path.getsize(de.FIXTURE), fx["liblz4"]))
    for c, fr in pairs:
        if (c, fr) not in forced:
            print("  not forced: %s %s: level 9 wrote %s, planted %s" % (c.name, fr, de.parse_of(c, fr, fx["cases"][c.name][fr]["seqs9"])[:4], c.expected(fr)[:4]))


if __name__ == "__main__":
    main()
