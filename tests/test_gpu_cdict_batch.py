"""The prepared dictionary of the batch encoder: lz4f_mi355x_dev_createCDict / lz4f_mi355x_dev_compressFrames_usingCDict
(Engine.create_cdict, compress_frames_async(..., cdict=), decompress_frames_async(..., dictionary=cdict)).

The yardstick throughout is lz4f_mi355x_dev_compressFrames_usingDict on the same engine with the same dictionary bytes - existing
code, held to liblz4 and to the dictionary model by tests/test_gpu_dict_batch.py.  A CDict's frames and records must be that
call's, byte for byte: the digest replaces a chunk's seeding only where the seeded table is a function of the dictionary alone."""
import numpy as np
import pytest
import torch

import dict_cases as dc
from alignment_cases import DST_RES, SRC_RES, carve, intact
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd.device import CDict, DeviceCodecError, Engine, frame_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 192
PAT = 0xA5
ST_DST_SMALL = 11


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    f = dc.load_fixture()
    dc.check_sha(f)
    return f


def _dev(b, extra: int = 0) -> torch.Tensor:
    a = np.frombuffer(bytes(b) + b"\0" * extra, dtype=np.uint8) if len(b) + extra else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a.copy()).to(DEV)


def _off(v) -> torch.Tensor:
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


def dev_bytes(b: bytes, res: int = 0) -> torch.Tensor:
    """b in device memory, `res` bytes past a 64-byte boundary."""
    view, _, _ = carve(len(b), res, device=DEV)
    if len(b): view.copy_(_dev(b))
    return view


_PREPARED = {}


def prepared(eng, dname: str):
    """(the dictionary in device memory, the engine's CDict of it): made once per dictionary, the CDict closed with the engine."""
    if dname not in _PREPARED or _PREPARED[dname][1].h is None or _PREPARED[dname][1].engine is not eng:
        d = dev_bytes(dc.dictionary(dname))
        _PREPARED[dname] = (d, eng.create_cdict(d))
    return _PREPARED[dname]


def prefs(linked=0, on=0, level=0, bsid=4):
    return conduit.make_preferences(blockSizeID=bsid, blockMode=0 if linked else 1, blockChecksum=on, contentChecksum=on,
                                    contentSize=1 if on else 0, dictID=77 if on else 0, compressionLevel=level)


class Encoded:
    """One batch compress: frame i in a window of its own (frame_windows + GUARD spare bytes, or `windows`), PAT before the call."""

    def __init__(self, eng, inputs, p, windows=None, src_res=0, dst_res=0, **how):
        lens = [len(x) for x in inputs]
        so = [0]
        for n in lens: so.append(so[-1] + n)
        if windows is None: do = frame_windows(lens, p, GUARD)
        else:
            do = [0]
            for w in windows: do.append(do[-1] + w)
        src, _, _ = carve(so[-1] + 16, src_res, device=DEV)
        src.copy_(_dev(b"".join(inputs), 16))
        dst, g0, g1 = carve(max(do[-1], 1), dst_res, device=DEV)
        res = eng.new_results(len(lens))
        eng.compress_frames_async(src, _off(so), dst, _off(do), p, res, **how)
        self.recs = eng.frame_results(res)
        out = dst.cpu().numpy().tobytes()
        assert intact(g0, g1)
        self.wins = [out[do[i]:do[i + 1]] for i in range(len(lens))]

    def frame(self, i) -> bytes:
        return self.wins[i][:self.recs[i].size]

    def untouched_behind(self) -> bool:
        return all(w[r.size:] == bytes([PAT]) * (len(w) - r.size) for w, r in zip(self.wins, self.recs))

    def all(self):
        return [(r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags, self.frame(i)) for i, r in enumerate(self.recs)]


def assert_equal_frames(eng, inputs, p, d: torch.Tensor, c: CDict, what):
    """Every frame's (status, size, consumed, n_blocks, first_bad_block, flags, bytes) with the CDict is _usingDict's, and nothing
    behind `size` is touched in any window.  -> the CDict's run"""
    want = Encoded(eng, inputs, p, dictionary=d)
    got = Encoded(eng, inputs, p, cdict=c)
    assert all(r.status == 0 for r in want.recs), what
    for i, (g, w) in enumerate(zip(got.all(), want.all())):
        assert g == w, (what, i, len(inputs[i]), g[:6], w[:6])
    assert got.untouched_behind(), what
    return got


def decoded(eng, frames, windows, dictionary):
    """One batch decode -> [(status, size, consumed, n_blocks, first_bad_block, flags, the window's bytes)]."""
    so, do = [0], [0]
    for f, w in zip(frames, windows):
        so.append(so[-1] + len(f)); do.append(do[-1] + w)
    dst = torch.full((max(do[-1], 1),), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(frames))
    eng.decompress_frames_async(_dev(b"".join(frames), 16), _off(so), dst, _off(do), res, dictionary=dictionary)
    recs = eng.frame_results(res)
    out = dst.cpu().numpy().tobytes()
    return [(r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags, out[do[i]:do[i + 1]]) for i, r in enumerate(recs)]


def measure(eng, frames) -> "list[int]":
    """The windows lz4f_mi355x_dev_measureFrames gives these frames (it never looks at offsets: no dictionary needed)."""
    so = [0]
    for f in frames: so.append(so[-1] + len(f))
    do = torch.zeros(len(frames) + 1, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(_dev(b"".join(frames), 16), _off(so), eng.new_results(len(frames)), do)
    eng.stream.synchronize()
    w = do.cpu().tolist()
    return [w[i + 1] - w[i] for i in range(len(frames))]


# ---- 1: equal frames ----
@pytest.mark.parametrize("on", (0, 1))
@pytest.mark.parametrize("linked", (0, 1))
@pytest.mark.parametrize("level", (0, 2))
@pytest.mark.parametrize("dname", list(dc.DICT_LEN))
def test_equal_frames(eng, dname, level, linked, on):
    d, c = prepared(eng, dname)
    assert c.size == min(dc.DICT_LEN[dname], dc.KB64)
    inputs = [x for _, x in dc.natural(dname)]
    if dname == "phrase": assert max(len(x) for x in inputs) == 131085            # (chunks and blocks behind the first)
    assert_equal_frames(eng, inputs, prefs(linked, on, level), d, c, (dname, level, linked, on))


# ---- 2: dictionary lengths at the seeding scheme's edges ----
EDGE_LENS = (4, 5, 7, 8, 15, 16, 17, 19, 20, 1023, 1024, 1025, 1027, 1040, 9215, 9216, 9217, 9232, 65535, 65536, 65537)
EDGE_RECORDS = (5, 13, 65, 300, 1000, 4096, 65536, 65537)


@pytest.mark.parametrize("n", EDGE_LENS)
def test_dictionary_lengths_at_the_seeding_edges(eng, n):
    """16-byte lanes, the dense last KiB, and the first full sparse round of 8 x 1024 bytes in front of it."""
    tail = dc.dictionary("big")[-n:]
    inputs = [dc.stitched("edge%d/%d" % (n, k), k, tail) for k in EDGE_RECORDS]
    d = dev_bytes(tail)
    with eng.create_cdict(d) as c:
        assert c.size == min(n, dc.KB64)
        for linked in (0, 1):
            got = assert_equal_frames(eng, inputs, prefs(linked, on=1 - linked), d, c, (n, linked))
            dec = decoded(eng, [got.frame(i) for i in range(len(inputs))], [len(x) for x in inputs], c)
            for i, x in enumerate(inputs):
                assert dec[i][0] == 0 and dec[i][1] == len(x) and dec[i][6] == x, (n, linked, len(x), dec[i][:6])


# ---- 3: chunks behind the first inside one block ----
@pytest.mark.parametrize("linked", (0, 1))
def test_chunks_behind_the_first_in_a_block(eng, linked):
    d, c = prepared(eng, "phrase")
    src = dc.tail(dc.dictionary("phrase"))
    inputs = [dc.stitched("inblock/%d" % n, n, src) for n in (65537, 131085, 200000)]
    got = assert_equal_frames(eng, inputs, prefs(linked, on=1, bsid=5), d, c, linked)
    assert [r.n_blocks for r in got.recs] == [1, 1, 1]


# ---- 4: the CDict owns its bytes and is not consumed ----
def test_cdict_owns_its_bytes_and_is_not_consumed(eng):
    intact_d = dev_bytes(dc.dictionary("phrase"))
    source = intact_d.clone()
    c = eng.create_cdict(source)
    eng.stream.synchronize()
    source.fill_(0xFF)
    torch.cuda.synchronize()
    try:
        nat = [x for _, x in dc.natural("phrase")]
        for k, (inputs, p) in enumerate(((nat[:20], prefs()), (nat[20:40], prefs(linked=1, on=1)), (nat[-6:], prefs(on=1, level=2)))):
            assert_equal_frames(eng, inputs, p, intact_d, c, k)
        assert bool((source == 0xFF).all())
    finally:
        c.close()


# ---- 5: alignment ----
def test_any_alignment(eng):
    """The dictionary the CDict is made from at byte residues 0, 1 and 3, source and destination at a handful of residues."""
    inputs = [x for _, x in dc.natural("d1k")] + [dc.stitched("align/70000", 70000, dc.tail(dc.dictionary("phrase")))]
    p = prefs(on=1)
    want = Encoded(eng, inputs, p, dictionary=dev_bytes(dc.dictionary("d1k"))).all()
    places = [(0, SRC_RES[0], DST_RES[0]), (1, SRC_RES[1], DST_RES[1]), (3, SRC_RES[3], DST_RES[2]), (1, SRC_RES[-1], DST_RES[-1]), (3, SRC_RES[7], DST_RES[3])]
    for dres, sres, tres in places:
        d = dev_bytes(dc.dictionary("d1k"), dres)
        assert d.data_ptr() % 64 == dres
        with eng.create_cdict(d) as c:
            got = Encoded(eng, inputs, p, cdict=c, src_res=sres, dst_res=tres)
            assert got.all() == want and got.untouched_behind(), (dres, sres, tres)


# ---- 6: isolation ----
def test_frames_are_isolated(eng):
    d, c = prepared(eng, "phrase")
    inputs = [x for _, x in dc.natural("phrase")]
    p = prefs(on=1)
    many = assert_equal_frames(eng, inputs, p, d, c, "many")
    for i in (0, 3, 9, 14, len(inputs) - 5, len(inputs) - 1):
        assert Encoded(eng, [inputs[i]], p, cdict=c).all()[0] == many.all()[i], i
    short = set(range(1, len(inputs), 4))
    tight = Encoded(eng, inputs, p, cdict=c, windows=[r.size - 1 if i in short else r.size for i, r in enumerate(many.recs)])
    for i in range(len(inputs)):
        if i in short:
            assert tight.recs[i].status == ST_DST_SMALL and tight.recs[i].size == 0 and tight.wins[i] == bytes([PAT]) * len(tight.wins[i]), i
        else:
            assert tight.all()[i] == many.all()[i], i


# ---- 7: decode with a CDict ----
@pytest.mark.parametrize("dname", ("phrase", "d1k"))
@pytest.mark.parametrize("mode", dc.MODES)
def test_decode_takes_a_cdict(eng, fx, dname, mode):
    """liblz4's frames and the planted ones: dictionary=cdict gives the verdicts and bytes of dictionary=tensor."""
    d, c = prepared(eng, dname)
    cases = dc.fixture_frames(fx, dname, mode)
    frames = [f for _, f, _, _ in cases]
    wins = measure(eng, frames)
    want = decoded(eng, frames, wins, d)
    assert decoded(eng, frames, wins, c) == want
    assert sum(1 for v in want if v[0] == 0) >= 8
    for (name, _, exp, _), v in zip(cases, want):
        if exp is not None: assert v[0] == 0 and v[6][:v[1]] == exp, name


# ---- 8: the edges of the contract ----
def test_no_cdict_and_empty_cdict_are_the_plain_call(eng):
    inputs = [x for _, x in dc.natural("phrase")]
    with eng.create_cdict(torch.zeros(0, dtype=torch.uint8, device=DEV)) as empty:
        assert empty.size == 0 and empty.data_ptr is None
        for linked in (0, 1):
            p = prefs(linked, on=1)
            plain = Encoded(eng, inputs, p).all()
            assert Encoded(eng, inputs, p, cdict=None).all() == plain
            assert Encoded(eng, inputs, p, cdict=empty).all() == plain
        frames = [f for _, f, exp, _ in dc.fixture_frames(dc.load_fixture(), "d1k", "indep")]
        assert decoded(eng, frames, [4096] * len(frames), empty) == decoded(eng, frames, [4096] * len(frames), None)


def _one_call(eng, p, **how):
    inputs = [x for _, x in dc.natural("d1k")]
    lens = [len(x) for x in inputs]
    so = [0]
    for n in lens: so.append(so[-1] + n)
    do = frame_windows(lens, p, GUARD)
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(lens))
    return (lambda e: e.compress_frames_async(_dev(b"".join(inputs), 16), _off(so), dst, _off(do), p, res, **how)), dst, res


@pytest.mark.parametrize("level", (3, 9))
def test_hc_levels_take_no_cdict(eng, level):
    _, c = prepared(eng, "d1k")
    call, dst, res = _one_call(eng, prefs(level=level), cdict=c)
    with pytest.raises(DeviceCodecError, match="compressionLevel_invalid"):
        call(eng)
    eng.stream.synchronize()
    assert bool((dst == PAT).all()) and not bool(res.any())


def test_cdict_of_another_engine_is_refused(eng):
    _, c = prepared(eng, "d1k")
    other = Engine(0)
    try:
        call, dst, res = _one_call(other, prefs(), cdict=c)
        with pytest.raises(DeviceCodecError, match="another engine"):
            call(other)
        torch.cuda.synchronize()
        assert bool((dst == PAT).all()) and not bool(res.any())
    finally:
        other.close()
    assert c.h is not None                                                      # (the other engine's close left it alone)


def test_arguments_are_checked(eng):
    d, c = prepared(eng, "d1k")
    call, dst, res = _one_call(eng, prefs(), cdict=c, dictionary=d)
    with pytest.raises(ValueError):
        call(eng)
    for bad in (torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.int32, device=DEV), b"abc", torch.zeros((2, 4), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            eng.create_cdict(bad)
        with pytest.raises(ValueError):
            _one_call(eng, prefs(), cdict=bad)[0](eng)
    eng.stream.synchronize()
    assert bool((dst == PAT).all()) and not bool(res.any())


def test_close_twice_and_a_closed_cdict(eng):
    c = eng.create_cdict(dev_bytes(dc.dictionary("d3")))
    assert c.size == 3 and c.data_ptr                                           # (kept for the decoder, ignored by the finder)
    c.close()
    c.close()
    assert c.h is None and c.size == 0
    with pytest.raises(ValueError):
        _one_call(eng, prefs(), cdict=c)[0](eng)
    # an engine closes the CDicts its caller forgot
    e2 = Engine(0)
    forgotten = e2.create_cdict(dev_bytes(dc.dictionary("d1k")))
    e2.close()
    assert forgotten.h is None
    forgotten.close()
