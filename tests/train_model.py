"""What lz4f_mi355x_dev_trainDict computes, as a sequential statement in plain numpy (test helper, not a test module).

The trainer picks the segments of a sample corpus whose d-byte substrings ("dmers") are the most frequent in the corpus, and lays
them right-aligned into the dictionary, the best ones last - where an LZ4 encoder's offsets are shortest.  The definition:

  corpus    C = the valid samples back to back (a span with src_off[i] > src_off[i+1] or an end past srcBytes gives nothing; a sample
            is taken only while the running total stays <= srcBytes, the first that does not fit ends the corpus).  N = len(C).
  hash      M = N - d + 1 dmers; h(j) = (the d bytes at C[j], little-endian, * 0x9E3779B185EBCA87 mod 2^64) >> (64 - f);
            freq[x] = the number of j with h(j) == x.
  windows   m = min(k - d + 1, M) dmers to a window, W = M - m + 1 window starts.  score(p; F) = the sum of F over the window's
            DISTINCT hashes: over the j in [p, p + m) whose previous occurrence prev(j) lies in front of p.
  epochs    E = max(1, min(dictSize // k, W)); epoch e holds the starts [e * W // E, (e + 1) * W // E).
  rounds    every round: S = a snapshot of freq; every epoch picks the lowest p with the best score(p; S); then, in epoch order, a
            pick with score 0 is skipped, a pick whose live score has fallen below half its snapshot score is stale and skipped (the
            epoch picks afresh in the next round), and any other is trimmed to its first and last dmer that still counts, appended
            in front of what the dictionary holds (cut to the room that is left, its beginning kept), and its dmers' counts zeroed.
            The rounds end when the dictionary is full, when a round appended nothing, or after `rounds` of them.

`train` is written for speed (a difference array and one running sum give every score of a round); `train_naive` is the definition
word for word, for the small cases the CPU test holds `train` to.  The two seeded corpora of tests/golden/train_dict_sizes.json
(tools/mint_train_dict_sizes.py) are built here too.
"""
from __future__ import annotations

import hashlib
from collections import namedtuple

import numpy as np

import dict_cases as dc

PRIME = 0x9E3779B185EBCA87
DEFAULTS = dict(k=64, d=8, f=18, rounds=16)          # the library's defaults (include/lz4f_mi355x.h)
PATH_BATCH = 0x1000                                    # LZ4F_MI355X_PATH_BATCH
NONE = 0xFFFFFFFF
KB64 = 65536

# dict: dictSize bytes; used, consumed (N), n_segments, first_bad, rounds_run: the record; log: (round, epoch, p, what) with what one
# of "zero", "stale", or the (s0, s1, take) of an appended segment
Trained = namedtuple("Trained", "dict used consumed n_segments first_bad rounds_run log")


def resolve(params: "dict | None") -> dict:
    """The call's parameters with the defaults where a field is 0 or missing."""
    p = dict(DEFAULTS)
    for key, v in (params or {}).items():
        if v: p[key] = int(v)
    return p


def corpus(src: bytes, off, src_bytes: "int | None" = None) -> "tuple[bytes, int]":
    """(C, first invalid sample or NONE) of the samples src[off[i]:off[i+1]]."""
    src_bytes = len(src) if src_bytes is None else src_bytes
    parts, total, bad, full = [], 0, NONE, False
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        if a > b or b > src_bytes:
            if bad == NONE: bad = i
            continue
        if full or total + (b - a) > src_bytes:
            full = True
            continue
        parts.append(src[a:b]); total += b - a
    return b"".join(parts), bad


def hashes(C: bytes, d: int, f: int) -> np.ndarray:
    c = np.frombuffer(C, dtype=np.uint8).astype(np.uint64)
    M = len(C) - d + 1
    v = np.zeros(M, dtype=np.uint64)
    for b in range(d):
        v |= c[b:b + M] << np.uint64(8 * b)
    with np.errstate(over="ignore"):
        return ((v * np.uint64(PRIME)) >> np.uint64(64 - f)).astype(np.int64)


def _shape(N: int, dict_size: int, k: int, d: int):
    M = N - d + 1
    m = min(k - d + 1, M)
    W = M - m + 1
    E = max(1, min(dict_size // k, W))
    return M, m, W, E


def _finish(C, dict_size, tail, pieces, n_seg, bad, rounds_run, log) -> Trained:
    body = b"".join(reversed(pieces))
    assert len(body) == dict_size - tail
    return Trained(bytes(tail) + body, dict_size - tail, len(C), n_seg, bad, rounds_run, log)


def train(C: bytes, dict_size: int, params: "dict | None" = None, first_bad: int = NONE) -> Trained:
    """The dictionary of corpus C (see the module's text)."""
    q = resolve(params)
    k, d, f, rounds = q["k"], q["d"], q["f"], q["rounds"]
    assert d in (4, 6, 8) and d <= k <= 4096 and 16 <= f <= 22 and 1 <= rounds <= 64 and 0 <= dict_size <= KB64
    N = len(C)
    if N < d or dict_size == 0:
        return Trained(bytes(dict_size), 0, N, 0, first_bad, 0, [])
    M, m, W, E = _shape(N, dict_size, k, d)
    h = hashes(C, d, f)
    freq = np.bincount(h, minlength=1 << f).astype(np.int64)
    j = np.arange(M, dtype=np.int64)
    order = np.argsort(h, kind="stable")
    prev = np.full(M, -1, dtype=np.int64)
    same = h[order[1:]] == h[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    dist = np.minimum(j - prev, m)                      # dmer j counts for the starts [j - dist + 1, j]
    lo = j - dist + 1
    inwin = np.arange(m, dtype=np.int64)
    tail, pieces, n_seg, log, rounds_run = dict_size, [], 0, [], 0
    for r in range(rounds):
        rounds_run += 1
        v = freq[h].astype(np.float64)                  # (sums stay far below 2^53: exact)
        diff = np.bincount(lo, weights=v, minlength=M + 1) - np.bincount(j + 1, weights=v, minlength=M + 1)
        score = np.cumsum(diff)[:W].astype(np.int64)
        picks = []
        for e in range(E):
            a, b = e * W // E, (e + 1) * W // E
            p = a + int(np.argmax(score[a:b]))          # (argmax: the first of equals)
            picks.append((p, int(score[p])))
        appended = 0
        for e, (p, s) in enumerate(picks):
            if s == 0:
                log.append((r, e, p, "zero")); continue
            hw = h[p:p + m]
            fw = freq[hw]
            live = int(fw[dist[p:p + m] > inwin].sum())
            if 2 * live < s:
                log.append((r, e, p, "stale")); continue
            on = np.nonzero(fw > 0)[0]
            s0, s1 = p + int(on[0]), p + int(on[-1])
            seg = C[s0:s1 + d]
            take = min(len(seg), tail)
            pieces.append(seg[:take]); tail -= take
            freq[h[s0:s1 + 1]] = 0
            n_seg += 1; appended += 1
            log.append((r, e, p, (s0, s1, take)))
            if tail == 0: break
        if tail == 0 or appended == 0: break
    return _finish(C, dict_size, tail, pieces, n_seg, first_bad, rounds_run, log)


def train_naive(C: bytes, dict_size: int, params: "dict | None" = None, first_bad: int = NONE) -> Trained:
    """The definition word for word: Python integers, sets for the distinct hashes, a window at a time.  For small inputs."""
    q = resolve(params)
    k, d, f, rounds = q["k"], q["d"], q["f"], q["rounds"]
    N = len(C)
    if N < d or dict_size == 0:
        return Trained(bytes(dict_size), 0, N, 0, first_bad, 0, [])
    M, m, W, E = _shape(N, dict_size, k, d)
    h = [((int.from_bytes(C[j:j + d], "little") * PRIME) & (2 ** 64 - 1)) >> (64 - f) for j in range(M)]
    freq: dict = {}
    for x in h: freq[x] = freq.get(x, 0) + 1
    score = lambda p, F: sum(F[x] for x in set(h[p:p + m]))
    tail, pieces, n_seg, log, rounds_run = dict_size, [], 0, [], 0
    for r in range(rounds):
        rounds_run += 1
        S = dict(freq)
        picks = []
        for e in range(E):
            best, at = -1, 0
            for p in range(e * W // E, (e + 1) * W // E):
                s = score(p, S)
                if s > best: best, at = s, p
            picks.append((at, best))
        appended = 0
        for e, (p, s) in enumerate(picks):
            if s == 0:
                log.append((r, e, p, "zero")); continue
            if 2 * score(p, freq) < s:
                log.append((r, e, p, "stale")); continue
            on = [jj for jj in range(p, p + m) if freq[h[jj]] > 0]
            s0, s1 = on[0], on[-1]
            seg = C[s0:s1 + d]
            take = min(len(seg), tail)
            pieces.append(seg[:take]); tail -= take
            for jj in range(s0, s1 + 1): freq[h[jj]] = 0
            n_seg += 1; appended += 1
            log.append((r, e, p, (s0, s1, take)))
            if tail == 0: break
        if tail == 0 or appended == 0: break
    return _finish(C, dict_size, tail, pieces, n_seg, first_bad, rounds_run, log)


def train_samples(src: bytes, off, dict_size: int, params: "dict | None" = None, src_bytes: "int | None" = None) -> Trained:
    """The call as the device takes it: samples by offsets."""
    C, bad = corpus(src, off, src_bytes)
    return train(C, dict_size, params, bad)


def record_flags(t: Trained) -> int:
    return PATH_BATCH << 12 | t.rounds_run


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


# ---- the two seeded corpora ----
CORPORA = ("uniform", "zipf")
N_TRAIN, N_HELD, REC = 2048, 256, 1024
_cache: dict = {}


def _zipf_records(n: int) -> "list[bytes]":
    r = dc.rng_of("train/zipf")
    pool = [bytes(r.integers(97, 123, int(k), dtype=np.uint8)) for k in r.integers(12, 60, 20000)]
    recs = []
    for _ in range(n):
        out = bytearray()
        while len(out) < REC:
            z = int(r.zipf(1.3))
            if z > len(pool): continue                  # (the distribution's far tail: drawn again)
            out += pool[z - 1]
            out += bytes(r.integers(0, 256, int(r.integers(0, 4)), dtype=np.uint8))
        recs.append(bytes(out[:REC]))
    return recs


def records(name: str) -> "tuple[list[bytes], list[bytes]]":
    """(the 2048 training records, the 256 held-out records) of a corpus, 1 KiB each."""
    if name not in _cache:
        if name == "uniform":
            src = dc.tail(dc.dictionary("phrase"))
            recs = [dc.stitched("train/uniform/%d" % i, REC, src) for i in range(N_TRAIN + N_HELD)]
        elif name == "zipf":
            recs = _zipf_records(N_TRAIN + N_HELD)
        else:
            raise KeyError(name)
        _cache[name] = (recs[:N_TRAIN], recs[N_TRAIN:])
    return _cache[name]


def offsets(recs) -> "list[int]":
    off = [0]
    for x in recs: off.append(off[-1] + len(x))
    return off


def naive_dictionary(name: str, dict_size: int) -> bytes:
    """The first dict_size bytes of the training samples as they come."""
    return b"".join(records(name)[0])[:dict_size]


def trained(name: str, dict_size: int, params: "dict | None" = None) -> Trained:
    key = ("trained", name, dict_size, tuple(sorted(resolve(params).items())))
    if key not in _cache:
        _cache[key] = train(b"".join(records(name)[0]), dict_size, params)
    return _cache[key]
