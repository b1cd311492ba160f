#!/usr/bin/env python3
"""Mint tests/golden/train_dict_sizes.json: what the dictionaries of tests/train_model.py are worth to liblz4.

Run on a machine that has liblz4 (>= 1.9.0: LZ4F_createCDict, LZ4F_compressFrame_usingCDict); the tests never need it.  For both
seeded corpora (uniform, zipf: 2048 training records and 256 held-out records of 1 KiB) and dictSize in {16 KiB, 64 KiB}, with the
library's default parameters, a row:
  sha256    of the model's dictionary (the device's must be the same bytes)
  none      liblz4's total over the held-out records, each an independent frame at level 0, with no dictionary
  naive     the same with the first dictSize bytes of the training samples as the dictionary
  trained   the same with the model's dictionary
And the table the defaults were chosen by: the same totals at dictSize 64 KiB for k in {64, 128, 256} and d in {6, 8} (f and rounds at
their defaults) - the pair with the smallest total over both corpora is what include/lz4f_mi355x.h names as LZ4F_MI355X_TRAIN_K and
LZ4F_MI355X_TRAIN_D, and what tests/train_model.py's DEFAULTS must say: this tool refuses to write a fixture otherwise.

    python tools/mint_train_dict_sizes.py [path to liblz4.so]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

import mint_dict_golden as mg     # noqa: E402
import train_model as tm          # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "train_dict_sizes.json")
SIZES = (16384, 65536)
GRID_K, GRID_D = (64, 128, 256), (6, 8)


def total(L, held, d: bytes) -> int:
    return sum(len(mg.compress(L, x, d, True)) for x in held)


def main():
    L = mg.liblz4(sys.argv[1] if len(sys.argv) > 1 else "liblz4.so.1")
    fx = {"liblz4": L.LZ4_versionString().decode(), "defaults": dict(tm.DEFAULTS), "rows": [], "grid": []}
    for name in tm.CORPORA:
        train, held = tm.records(name)
        fx.setdefault("corpora", {})[name] = {"train_sha256": tm.sha(b"".join(train)), "held_sha256": tm.sha(b"".join(held))}
        none = total(L, held, b"")
        for size in SIZES:
            t = tm.trained(name, size)
            fx["rows"].append({"corpus": name, "dict_size": size, "sha256": tm.sha(t.dict), "used": t.used, "segments": t.n_segments, "rounds": t.rounds_run,
                               "none": none, "naive": total(L, held, tm.naive_dictionary(name, size)), "trained": total(L, held, t.dict)})
        for k in GRID_K:
            for d in GRID_D:
                t = tm.trained(name, 65536, {"k": k, "d": d})
                fx["grid"].append({"corpus": name, "k": k, "d": d, "trained": total(L, held, t.dict), "rounds": t.rounds_run})
    by_pair = {}
    for g in fx["grid"]:
        by_pair[(g["k"], g["d"])] = by_pair.get((g["k"], g["d"]), 0) + g["trained"]
    best = min(by_pair, key=lambda kd: (by_pair[kd], kd))
    for g in fx["grid"]:
        print("  %-8s k=%-4d d=%d  %7d bytes  %2d rounds" % (g["corpus"], g["k"], g["d"], g["trained"], g["rounds"]))
    print("totals:", {"k=%d d=%d" % kd: v for kd, v in sorted(by_pair.items())}, "-> best", best)
    if best != (tm.DEFAULTS["k"], tm.DEFAULTS["d"]):
        print("the defaults are k=%d d=%d: change them (include/lz4f_mi355x.h, device.py, tests/train_model.py) and mint again" % (tm.DEFAULTS["k"], tm.DEFAULTS["d"]))
        return 1
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write("\n")
    for r in fx["rows"]:
        print("  %-8s %5d: none %d, naive %d, trained %d (%d segments, %d rounds)" % (r["corpus"], r["dict_size"], r["none"], r["naive"], r["trained"], r["segments"], r["rounds"]))
    print("%s: %d bytes; liblz4 %s" % (os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), fx["liblz4"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
