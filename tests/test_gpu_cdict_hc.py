"""The prepared dictionary at levels 3-12: lz4f_mi355x_dev_createCDictHC / Engine.create_cdict(d, hc=True) gives the CDict the
hash-chain finder's digest, and lz4f_mi355x_dev_compressFrames_usingCDict then searches the dictionary at those levels.

Held to: the dictionary model (dict_cases.model_decode, CPU, the oracle's block decoder) and the device's own dictionary decoder for
what the frames decode to; the block format's writer rules; the plain calls of the same engine for what must not change; and, in
size, liblz4's totals in tests/golden/dict_hc_sizes.json (tools/mint_dict_hc_sizes.py)."""
import json
import os

import pytest
import torch

import dict_cases as dc
from lz4_frame_conduit_amd.device import DeviceCodecError, Engine
from test_gpu_cdict_batch import DEV, PAT, Encoded, _one_call, decoded, dev_bytes, prefs
from test_gpu_dict_batch import check_writer_rules

pytestmark = pytest.mark.gpu
SIZES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dict_hc_sizes.json")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


_HC = {}


def hc_prepared(eng, dname: str):
    """(the dictionary's bytes, the engine's HC CDict of them): made once per dictionary, closed with the engine."""
    if dname not in _HC or _HC[dname][1].h is None or _HC[dname][1].engine is not eng:
        d = dc.dictionary(dname)
        _HC[dname] = (d, eng.create_cdict(dev_bytes(d), hc=True))
    return _HC[dname]


def round_trip(eng, inputs, p, d: bytes, c, what) -> Encoded:
    """One call through the HC CDict: every status 0, nothing behind `size` touched (Encoded checks the guards), the model and the
    device's dictionary decoder (with the CDict's own copy) give the inputs back, the writer rules hold.  -> the run"""
    got = Encoded(eng, inputs, p, cdict=c)
    assert got.untouched_behind(), what
    frames = [got.frame(i) for i in range(len(inputs))]
    for i, x in enumerate(inputs):
        r = got.recs[i]
        assert (r.status, r.consumed) == (0, len(x)), (what, i, len(x), r.status)
        v = dc.model_decode(frames[i], d)
        assert v.ok and v.out == x and v.consumed == r.size, (what, i, len(x), v.why)
        check_writer_rules(frames[i], min(len(d), dc.KB64), (what, i))
    dec = decoded(eng, frames, [max(len(x), 1) for x in inputs], c)
    for i, x in enumerate(inputs):
        assert dec[i][0] == 0 and dec[i][1] == len(x) and dec[i][6][:len(x)] == x, (what, i, len(x), dec[i][:6])
    return got


# ---- 1: round trip ----
@pytest.mark.parametrize("on", (0, 1))
@pytest.mark.parametrize("linked", (0, 1))
@pytest.mark.parametrize("level", (3, 6, 12))
@pytest.mark.parametrize("dname", ("d1", "d3", "d1k", "phrase", "big"))
def test_round_trip(eng, dname, level, linked, on):
    d, c = hc_prepared(eng, dname)
    assert c.hc and c.size == min(len(d), dc.KB64)
    inputs = [x for _, x in dc.natural(dname)]
    if dname == "phrase": assert sorted(len(x) for x in inputs)[-4:] == [65535, 65536, 65537, 131085]
    round_trip(eng, inputs, prefs(linked, on, level), d, c, (dname, level, linked, on))


# ---- 2: the seam and the batch edges ----
EDGE_LENS = (4, 5, 8, 959, 960, 961, 1919, 1920, 1921, 65535, 65536)          # HC_T = 960, two batches, the ring's reach


def edge_dictionary(n: int) -> bytes:
    """The last n bytes of the phrase dictionary; of `big` where the phrase dictionary (65 525 bytes) is too short."""
    return dc.dictionary("big" if n > dc.DICT_LEN["phrase"] else "phrase")[-n:]


def edge_record(n: int, d: bytes) -> bytes:
    """The dictionary's last bytes (a match that ends at the seam), its first ones, then 200 bytes stitched from the dictionary
    itself.  The first ones stand at position 40, n + 40 bytes behind their source: the farthest position there is while
    n + 40 <= 65535 - from n = 65496 on (the 65535- and 65536-byte dictionaries) they are out of reach and no match at all.  The
    reach edge itself (a source exactly 65535 back, and 65536) is test_gpu_dict_encoder_edges.py's."""
    k = min(40, n)
    return d[-k:] + d[:k] + dc.stitched("hcedge/%d" % n, 200, d)


@pytest.mark.parametrize("level", (3, 9))
@pytest.mark.parametrize("n", EDGE_LENS)
def test_dictionary_lengths_at_the_batch_edges(eng, n, level):
    d = edge_dictionary(n)
    assert len(d) == n
    x = edge_record(n, d)
    with eng.create_cdict(dev_bytes(d), hc=True) as c:
        for linked in (0, 1):
            p = prefs(linked, on=1 - linked, level=level)
            got = round_trip(eng, [x], p, d, c, (n, level, linked))
            if n >= 959:
                plain = Encoded(eng, [x], p)
                print("dictionary of %d bytes, level %d: %d bytes with it, %d without" % (n, level, got.recs[0].size, plain.recs[0].size))
                assert got.recs[0].size < plain.recs[0].size, (n, level, linked)


@pytest.mark.parametrize("level", (3, 9))
@pytest.mark.parametrize("name", ("double_tail", "long_slice"))
def test_matches_end_at_the_seam_and_long_ones_read_the_dictionary(eng, name, level):
    """d[-600:] twice: a match that runs to the dictionary's last byte and is cut there.  d[1000:1700]: a verbatim slice longer than
    a search records (258 bytes), so the parse's wave-wide extension reads the dictionary."""
    d, c = hc_prepared(eng, "phrase")
    x = d[-600:] + d[-600:] if name == "double_tail" else d[1000:1700]
    for linked in (0, 1):
        p = prefs(linked, on=linked, level=level)
        got = round_trip(eng, [x], p, d, c, (name, level, linked))
        plain = Encoded(eng, [x], p)
        print("%s, level %d: %d bytes with the dictionary, %d without" % (name, level, got.recs[0].size, plain.recs[0].size))
        assert got.recs[0].size < plain.recs[0].size, (name, level, linked)
        if name == "double_tail":
            blocks = dc.walk(got.frame(0))["blocks"]
            seqs = list(dc.sequences(got.frame(0)[blocks[0][1]:blocks[0][1] + blocks[0][2]]))
            assert seqs[0] == (0, 600, 600), seqs[:2]                             # the whole tail, and not a byte across the seam


# ---- 3: a function of its inputs ----
def test_frames_are_a_function_of_their_inputs(eng):
    d, c = hc_prepared(eng, "phrase")
    small = [x for _, x in dc.natural("phrase") if len(x) <= dc.RATIO_MAX]
    big = [x for _, x in dc.natural("phrase") if len(x) == 65537]
    kib = [dc.stitched("fn/%d" % k, 1024, dc.tail(d)) for k in range(6)]
    other = Engine(0)
    try:
        c2 = other.create_cdict(dev_bytes(d), hc=True)
        for level, linked in ((3, 0), (9, 1)):
            p = prefs(linked, on=1, level=level)
            many = Encoded(eng, small, p, cdict=c).all()
            assert all(v[0] == 0 for v in many)
            assert Encoded(eng, small, p, cdict=c).all() == many                  # two runs
            assert Encoded(other, small, p, cdict=c2).all() == many               # two engines, each with its own HC CDict
            assert Encoded(eng, small[::-1], p, cdict=c).all() == many[::-1]      # the batch in reversed order
            for i in range(len(small)):                                           # a batch of one, every record
                assert Encoded(eng, [small[i]], p, cdict=c).all()[0] == many[i], (level, i)
            # 1 KiB records between 65 537-byte ones (a workgroup per chunk here; test_a_workgroup_goes_from_chunk_to_chunk has more
            # chunks than workgroups)
            mixed = [kib[0], big[0], kib[1], kib[2], big[0], kib[3], big[0], big[0], kib[4], kib[5]]
            alone = {id(x): Encoded(eng, [x], p, cdict=c).all()[0] for x in kib + big}
            got = Encoded(eng, mixed, p, cdict=c).all()
            assert got == [alone[id(x)] for x in mixed], level
            assert Encoded(eng, mixed[::-1], p, cdict=c).all() == got[::-1], level
    finally:
        other.close()


FIND_GRID = 2048        # the most workgroups the hash-chain find kernels are launched with (engine.hip: BATCH_GRID / 4): workgroup b
                        # takes chunks b, b + 2048, ... of the chunk table, one after the other in the same LDS


@pytest.mark.parametrize("level,linked", ((3, 0), (9, 1)))
def test_a_workgroup_goes_from_chunk_to_chunk(eng, level, linked):
    """More chunks than workgroups in one call, so a workgroup loads the digest into LDS that an earlier chunk left dirty.  A
    65 537-byte record's first chunk ends at position 65 525 + 65 536 > HC_RING: it wraps the ring and overwrites chain slots below
    D.  Such records stand at the front (chunk b wraps, chunk b + 2048 is a 1 KiB record's) and at the end (the same once the batch
    is reversed; as it stands, a big chunk behind a small one).  Every frame is the one its record gets alone."""
    d, c = hc_prepared(eng, "phrase")
    big = [x for _, x in dc.natural("phrase") if len(x) == 65537][0]
    distinct = [dc.stitched("chunk2chunk/%d" % k, 1024 + (k * 37) % 512 if k % 4 else 300 + 61 * k, dc.tail(d)) for k in range(48)]
    p = prefs(linked, on=1, level=level)
    alone = {id(x): Encoded(eng, [x], p, cdict=c).all()[0] for x in distinct + [big]}
    assert all(v[0] == 0 for v in alone.values())
    front = [distinct[0], big, distinct[1], distinct[2], big, distinct[3], big, big, distinct[4]]
    body = [distinct[k % len(distinct)] for k in range(FIND_GRID + 100)]
    batch = front + body + [big, distinct[5], big, big, distinct[6]]
    chunks = sum(2 if x is big else 1 for x in batch)
    assert chunks > FIND_GRID + len(front) + 4 + 7                                # every big chunk has a chunk 2048 entries behind or in front
    got = Encoded(eng, batch, p, cdict=c).all()
    want = [alone[id(x)] for x in batch]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (level, linked, i, len(batch[i]), g[:6], w[:6])
    back = Encoded(eng, batch[::-1], p, cdict=c).all()
    for i, (g, w) in enumerate(zip(back, want[::-1])):
        assert g == w, (level, linked, "reversed", i, g[:6], w[:6])


# ---- 4: superset and refusals ----
@pytest.mark.parametrize("level", (0, 2))
def test_levels_up_to_2_are_the_plain_cdict(eng, level):
    d, c = hc_prepared(eng, "phrase")
    inputs = [x for _, x in dc.natural("phrase")]
    with eng.create_cdict(dev_bytes(d)) as plain_c:
        assert not plain_c.hc and c.hc
        for linked in (0, 1):
            p = prefs(linked, on=1, level=level)
            want = Encoded(eng, inputs, p, cdict=plain_c).all()
            assert all(v[0] == 0 for v in want)
            assert Encoded(eng, inputs, p, cdict=c).all() == want, (level, linked)


@pytest.mark.parametrize("level", (3, 9))
def test_dictionaries_the_finder_ignores_give_the_plain_call(eng, level):
    inputs = [x for _, x in dc.natural("d1k")] + [x for _, x in dc.natural("phrase") if len(x) == 65537]
    for d in (b"", b"x", b"abc"):
        with eng.create_cdict(dev_bytes(d) if d else torch.zeros(0, dtype=torch.uint8, device=DEV), hc=True) as c:
            assert c.hc and c.size == len(d)
            for linked in (0, 1):
                p = prefs(linked, on=1, level=level)
                want = Encoded(eng, inputs, p).all()
                assert all(v[0] == 0 for v in want)
                assert Encoded(eng, inputs, p, cdict=c).all() == want, (len(d), level, linked)


def test_hc_cdict_of_another_engine_is_refused(eng):
    _, c = hc_prepared(eng, "d1k")
    other = Engine(0)
    try:
        call, dst, res = _one_call(other, prefs(level=3), cdict=c)
        with pytest.raises(DeviceCodecError, match="another engine"):
            call(other)
        torch.cuda.synchronize()
        assert bool((dst == PAT).all()) and not bool(res.any())
    finally:
        other.close()
    assert c.h is not None


def test_has_hc(eng):
    d = dev_bytes(dc.dictionary("d1k"))
    with eng.create_cdict(d) as a, eng.create_cdict(d, hc=True) as b:
        L = eng.L
        assert L.lz4f_mi355x_cdict_has_hc(a.h) == 0 and L.lz4f_mi355x_cdict_has_hc(b.h) == 1
        assert a.hc is False and b.hc is True
        assert a.size == b.size == 1024 and a.data_ptr != b.data_ptr
    assert b.hc is False                                                          # (closed)


# ---- 5: ratio ----
@pytest.mark.parametrize("level", (3, 9, 12))
def test_ratio_against_liblz4(eng, level):
    """A condition, not a measured constant: over the ratio corpus the device's total with the HC CDict is at most halfway between
    liblz4's level-0 total with the dictionary and liblz4's total with the dictionary at this level - the device recovers at least
    half of what the chain search adds over the fast finder."""
    with open(SIZES) as f:
        fx = json.load(f)
    d, c = hc_prepared(eng, "phrase")
    assert dc.sha(d) == fx["dict"]["sha256"]
    inputs = [x for _, x in dc.natural("phrase") if len(x) <= dc.RATIO_MAX]
    assert len(inputs) == fx["records"] == 49 and [dc.sha(x) for x in inputs] == [e["sha256"] for e in fx["inputs"]]
    enc = Encoded(eng, inputs, prefs(level=level), cdict=c)
    plain = Encoded(eng, inputs, prefs(level=level))
    assert all(r.status == 0 for r in enc.recs)
    total, without = sum(r.size for r in enc.recs), sum(r.size for r in plain.recs)
    t0, t = fx["totals"]["0"]["with"], fx["totals"][str(level)]
    print("level %d: device with the HC CDict %d, without a dictionary %d; liblz4 with %d (x%.3f), without %d; liblz4 level 0 with %d" % (
        level, total, without, t["with"], total / t["with"], t["without"], t0))
    assert total <= (t0 + t["with"]) / 2, (level, total, t0, t["with"])
