"""The small cases of lz4f_mi355x_dev_trainDict: the smallest shapes at which each rule of the definition (tests/train_model.py) can
go wrong (test helper, not a test module; numpy only).  tests/test_train_model_cpu.py holds every case to what it was built to
show - by the model's log - and the fast model to the naive one; tests/test_gpu_train_dict.py holds the device to the model on them.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import dict_cases as dc
import train_model as tm

TILE, SCAN_TILE = 4096, 1024                     # LZ4F_MI355X_TRAIN_TILE, LZ4F_MI355X_TRAIN_SCAN_TILE (the CPU test holds them to the header)
P = dict(k=16, d=4, f=16, rounds=16)             # the cases' parameters unless a case says otherwise

# src: the sample buffer; off: n + 1 offsets; src_bytes: the call's srcBytes (None: len(src)); naive: small enough for train_naive
Case = namedtuple("Case", "name src off dict_size params src_bytes naive")


def case(name, src, off, dict_size, naive=True, src_bytes=None, **params) -> Case:
    return Case(name, bytes(src), [int(x) for x in off], dict_size, dict(P, **params), src_bytes, naive)


def text(name: str, n: int) -> bytes:
    """n bytes of phrases with repeats: stitched from the first 600 bytes of the phrase dictionary."""
    return dc.stitched("train/" + name, n, dc.dictionary("phrase")[:600], (8, 40))


def noise(name: str, n: int) -> bytes:
    return dc.rng_of("train/noise/" + name).integers(0, 256, n, dtype=np.uint8).tobytes()


def cut(data: bytes, sizes) -> "list[int]":
    """offsets that cut data into samples of the given sizes, over and over"""
    off, i = [0], 0
    while off[-1] < len(data):
        off.append(min(off[-1] + sizes[i % len(sizes)], len(data))); i += 1
    return off


def stale_plant() -> Case:
    """Two epochs.  H lies once in epoch 0 and twice in epoch 1, B twice in epoch 1, everything else once: both epochs pick H, epoch
    0 commits it, epoch 1's pick is stale and it takes B a round later."""
    r = lambda tag, n: noise("stale/" + tag, n)
    H, B = r("H", 16), r("B", 16)
    C = r("0", 40) + H + r("1", 44) + r("2", 30) + H + r("3", 10) + H + r("4", 9) + B + r("5", 10) + B + r("6", 20)
    return case("stale/planted", C, [0, len(C)], 47)


def tie_cases() -> "list[Case]":
    X = noise("tie/X", 40)
    out = [case("tie/one_epoch", noise("tie/a", 9) + X + noise("tie/b", 21) + X + noise("tie/c", 7), [0, 9 + 40 + 21 + 40 + 7], 20)]
    # across an epoch seam: two epochs, the same content in both; and the pad in front chosen so that epoch 0's pick is its last start
    for pad in range(100, 140):
        C = noise("tie/p", pad) + X[:16] + noise("tie/q", 70) + X[:16] + noise("tie/r", 30)
        M, m, W, E = tm._shape(len(C), 40, 16, 4)
        t = tm.train(C, 40, P)
        first = [x for x in t.log if x[0] == 0]
        if E == 2 and first[0][2] == W // 2 - 1 and first[0][3] not in ("zero", "stale"):
            out.append(case("tie/epoch_last_start", C, [0, len(C)], 40))
            break
    C = noise("tie/s", 30) + X[:16] + noise("tie/t", 60) + X[:16] + noise("tie/u", 30)
    out.append(case("tie/across_seam", C, [0, len(C)], 40))
    return out


_cases = None


def all_cases() -> "list[Case]":
    global _cases
    if _cases is not None: return _cases
    out = []
    one = lambda data: [0, len(data)]
    t600 = text("t600", 600)
    out.append(case("n/below_d", b"abc", [0, 1, 3], 64))
    out.append(case("n/equals_d", b"abcd", [0, 4], 64))
    for n in (15, 16, 17):
        out.append(case("n/k%+d" % (n - 16), text("nk", n), [0, n], 64))
    out.append(case("small_corpus", text("small", 200), one(bytes(200)), 1000))
    for ds in (1, 15, 16, 17, 53):
        out.append(case("dict_size/%d" % ds, t600, one(t600), ds))
    out.append(case("rounds/1", t600, one(t600), 300, rounds=1))
    out.append(case("rounds/2", t600, one(t600), 600, rounds=2))
    s256 = text("same", 256)
    out.append(case("same_sample_x64", s256 * 64, range(0, 64 * 256 + 1, 256), 1024, naive=False))
    out.append(case("one_byte_4k", b"\x41" * 4096, [0, 4096], 256, naive=False))
    out += tie_cases()
    out.append(stale_plant())
    n64 = noise("64k", 65536)
    out.append(case("noise_64k", n64, range(0, 65537, 1024), 4096, naive=False))
    out.append(case("seams/in_dmers", t600, cut(t600, (1, 2, 3, 5, 7, 11)), 200))
    out.append(case("seams/in_segments", t600, cut(t600, (9, 30, 17)), 200))
    out.append(case("empty_between", t600, [0, 0, 100, 100, 100, 350, 350, 600, 600], 200))
    # spans: overlapping, a reversed pair, one past srcBytes, descending addresses; and overlaps that overrun srcBytes (the rest dropped)
    out.append(case("spans/overlap", t600, [0, 300, 100, 400, 400, 600], 200))                   # (300 -> 100 is a reversed pair too)
    out.append(case("spans/reversed_and_past", t600 + bytes(40), [0, 200, 150, 700, 300, 600], 200, src_bytes=600))
    out.append(case("spans/descending", t600, [400, 600, 200, 400, 0, 200], 200))
    out.append(case("spans/overrun", t600, [0, 600, 0, 0, 1, 600, 0, 10], 200))
    for d, f in ((6, 16), (8, 17), (4, 22), (8, 22)):
        out.append(case("params/d%d_f%d" % (d, f), t600, cut(t600, (50,)), 150, d=d, f=f))
    out.append(case("params/k_equals_d", t600, one(t600), 64, k=8, d=8))
    big = text("tiles", 3 * TILE + 200)
    # one byte either side of the kernels' tile: the corpus' bytes, its dmers (N - 3), its window starts (N - 15)
    for what, add in (("bytes", 0), ("dmers", 3), ("starts", 15)):
        for delta in (-1, 0, 1):
            n = TILE + add + delta
            out.append(case("tile/%s%+d" % (what, delta), big[:n], cut(big[:n], (1000,)), 512, naive=False))
    out.append(case("tile/three_and_a_bit", big, cut(big, (777,)), 2048, naive=False))
    out.append(case("tile/k4096", big, cut(big, (1000,)), 8192 + 100, naive=False, k=4096))
    out.append(case("tile/k4096_d8", big, one(big), 4096, naive=False, k=4096, d=8))
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 5):
        data = text("scan", 3 * n)
        out.append(case("scan/%d_samples" % n, data, range(0, 3 * n + 1, 3), 256, naive=False))
    _cases = out
    assert len({c.name for c in out}) == len(out)
    return out


def by_name(name: str) -> Case:
    return {c.name: c for c in all_cases()}[name]


def model(c: Case) -> tm.Trained:
    return tm.train_samples(c.src, c.off, c.dict_size, c.params, c.src_bytes)
