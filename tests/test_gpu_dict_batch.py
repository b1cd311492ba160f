"""The batch calls with a shared dictionary: lz4f_mi355x_dev_decompressFrames_usingDict / lz4f_mi355x_dev_compressFrames_usingDict
(Engine.decompress_frames_async / compress_frames_async with dictionary=).

Decode is held to liblz4: its frames made with a CDict and its verdicts on the planted frames are in tests/golden/dict_frames.json
(tools/mint_dict_golden.py), rebuilt and checked by dict_cases.py.  Encode is held to the dictionary model (dict_cases.model_decode),
to the device's own dictionary decoder, to the block format's writer rules and - in size - to liblz4's totals in the fixture."""
import numpy as np
import pytest
import torch

import dict_cases as dc
from alignment_cases import DST_RES, SRC_RES, carve, intact
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd.device import DeviceCodecError, Engine, frame_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_BATCH = 0x1000
GUARD = 192
PAT = 0xA5
NONE = 0xFFFFFFFF
ST_GENERIC, ST_DST_SMALL, ST_HEADER_INCOMPLETE = 1, 11, 12
MFLIMIT, LASTLIT = 12, 5


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


_DICTS = {}


def dev_dict(dname: str, res: int = 0) -> torch.Tensor:
    """The dictionary in device memory, `res` bytes past a 64-byte boundary."""
    if (dname, res) not in _DICTS:
        view, _, _ = carve(dc.DICT_LEN[dname], res, device=DEV)
        view.copy_(_dev(dc.dictionary(dname)))
        _DICTS[(dname, res)] = view
    return _DICTS[(dname, res)]


def measure(eng, frames) -> "list[int]":
    """The windows lz4f_mi355x_dev_measureFrames gives these frames (it never looks at offsets: no dictionary needed)."""
    so = [0]
    for f in frames: so.append(so[-1] + len(f))
    do = torch.zeros(len(frames) + 1, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(_dev(b"".join(frames), 16), _off(so), eng.new_results(len(frames)), do)
    eng.stream.synchronize()
    d = do.cpu().tolist()
    return [d[i + 1] - d[i] for i in range(len(frames))]


class Decoded:
    """One batch decode: frame i's span is frames[i], its window windows[i] bytes; between the windows lie guard windows of frames
    with empty spans (frameHeader_incomplete: nothing may be written for them), PAT before the call.  src / dst may be views at
    any address (alignment test)."""

    def __init__(self, eng, frames, windows, dictionary, src_res=0, dst_res=0):
        so, do, real = [0], [0], []
        for f, c in zip(frames, windows):
            so.append(so[-1]); do.append(do[-1] + GUARD)
            real.append(len(so) - 1)
            so.append(so[-1] + len(f)); do.append(do[-1] + c)
        so.append(so[-1]); do.append(do[-1] + GUARD)
        src, _, _ = carve(so[-1] + 16, src_res, device=DEV)
        src.copy_(_dev(b"".join(frames), 16))
        dst, g0, g1 = carve(do[-1], dst_res, device=DEV)
        res = eng.new_results(len(so) - 1)
        eng.decompress_frames_async(src, _off(so), dst, _off(do), res, dictionary=dictionary)
        recs = eng.frame_results(res)
        out = dst.cpu().numpy().tobytes()
        assert intact(g0, g1)
        is_real = set(real)
        for k in range(len(recs)):
            if k not in is_real:
                assert recs[k].status == ST_HEADER_INCOMPLETE and out[do[k]:do[k + 1]] == bytes([PAT]) * GUARD, k
        self.recs = [recs[k] for k in real]
        self.wins = [out[do[k]:do[k + 1]] for k in real]

    def out(self, i) -> bytes:
        return self.wins[i][:self.recs[i].size]

    def verdicts(self):
        return [(r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags, self.out(i) if r.status == 0 else None) for i, r in enumerate(self.recs)]


def check_decoded(dec: Decoded, cases, windows):
    """Every frame against liblz4's verdict: accepted -> the recorded bytes, size, consumed, n_blocks, nothing behind `size`
    changed; rejected -> ERROR_GENERIC at liblz4's block."""
    for i, (name, frame, exp, bad) in enumerate(cases):
        r = dec.recs[i]
        assert r.flags >> 12 == PATH_BATCH, name
        if exp is not None:
            f = dc.walk(frame)
            assert (r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block) == (0, len(exp), f["consumed"], len(f["blocks"]), NONE), (name, r.status, r.size, r.first_bad_block)
            assert dec.out(i) == exp, name
            assert r.flags & 0xFF == f["flg"], name
        else:
            assert (r.status, r.first_bad_block) == (ST_GENERIC, bad), (name, r.status, r.first_bad_block, bad)


DECODE_SETS = [(d, m) for d in dc.DICT_LEN for m in dc.MODES]


@pytest.mark.parametrize("dname,mode", DECODE_SETS)
def test_decode_liblz4_frames(eng, fx, dname, mode):
    """1 + 2: liblz4's frames and the planted ones, one call per dictionary and block mode, in the tight windows measure gives
    them; and the same batch without the dictionary, which must reject exactly the frames that reach into it."""
    cases = dc.fixture_frames(fx, dname, mode)
    frames = [c[1] for c in cases]
    assert any(c[2] is None for c in cases) or dc.DICT_LEN[dname] + 11 > 65535
    wins = measure(eng, frames)
    dec = Decoded(eng, frames, wins, dev_dict(dname))
    check_decoded(dec, cases, wins)
    # without the dictionary: what the model says without one - the frames that reach into it fail, the others are untouched
    plain = Decoded(eng, frames, wins, None)
    reach = 0
    for i, (name, frame, exp, bad) in enumerate(cases):
        v = dc.model_decode(frame, b"")
        r = plain.recs[i]
        assert (r.status == 0) == v.ok, (name, r.status)
        if v.ok: assert plain.out(i) == v.out == exp, name
        else:
            assert (r.status, r.first_bad_block) == (ST_GENERIC, v.bad_block), (name, r.status, r.first_bad_block)
            reach += exp is not None
    assert reach >= 8, "the fixture's frames do not reach into the dictionary"


def test_window_one_byte_short_fails_alone(eng, fx):
    cases = [c for c in dc.fixture_frames(fx, "phrase", "indep") + dc.fixture_frames(fx, "phrase", "linked") if c[2]]
    frames = [c[1] for c in cases]
    wins = measure(eng, frames)
    short = set(range(0, len(frames), 3))
    dec = Decoded(eng, frames, [w - 1 if i in short else w for i, w in enumerate(wins)], dev_dict("phrase"))
    for i, (name, frame, exp, bad) in enumerate(cases):
        if i in short: assert dec.recs[i].status == ST_DST_SMALL, (name, dec.recs[i].status)
        else: assert dec.recs[i].status == 0 and dec.out(i) == exp, name


# ---- encode ----
def prefs(linked=0, bck=0, cck=0, csize=0, dictid=0, level=0):
    return conduit.make_preferences(blockSizeID=4, blockMode=0 if linked else 1, blockChecksum=bck, contentChecksum=cck,
                                    contentSize=1 if csize else 0, dictID=dictid, compressionLevel=level)


class Encoded:
    def __init__(self, eng, inputs, p, dictionary, windows=None, src_res=0, dst_res=0, plain_call=False):
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
        if plain_call: eng.compress_frames_async(src, _off(so), dst, _off(do), p, res)
        else: eng.compress_frames_async(src, _off(so), dst, _off(do), p, res, dictionary=dictionary)
        self.recs = eng.frame_results(res)
        out = dst.cpu().numpy().tobytes()
        assert intact(g0, g1)
        self.wins = [out[do[i]:do[i + 1]] for i in range(len(lens))]

    def frame(self, i) -> bytes:
        return self.wins[i][:self.recs[i].size]

    def untouched_behind(self, i) -> bool:
        n = self.recs[i].size
        return self.wins[i][n:] == bytes([PAT]) * (len(self.wins[i]) - n)

    def all(self):
        return [(r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags, self.frame(i)) for i, r in enumerate(self.recs)]


def check_writer_rules(frame: bytes, D: int, name):
    """The dictionary-aware walk: every offset within its scope + the dictionary, the last 5 bytes of a block literals, no match
    starting within its last 12."""
    f = dc.walk(frame)
    done = 0
    for stored, at, n in f["blocks"]:
        if stored:
            done += n
            continue
        pos = 0
        seqs = list(dc.sequences(frame[at:at + n]))
        blen = sum(l + m for l, m, _ in seqs)
        for lit, mlen, off in seqs:
            pos += lit
            if mlen == 0: break
            scope = pos + (min(done, dc.KB64) if f["linked"] else 0)
            assert 0 < off <= scope + D, (name, "offset", off, scope, D)
            assert pos + MFLIMIT <= blen and pos + mlen + LASTLIT <= blen, (name, "end rules", pos, mlen, blen)
            pos += mlen
        assert seqs[-1][1] == 0 and (len(seqs) == 1 or seqs[-1][0] >= LASTLIT), name
        done += blen


ENCODE_SETS = [("phrase", lv, linked, on) for lv in (0, 2) for linked in (0, 1) for on in (0, 1)] + [(d, 0, d == "d1k", 1) for d in ("d1", "d3", "d1k", "big")]


@pytest.mark.parametrize("dname,level,linked,on", ENCODE_SETS)
def test_encode_with_dictionary(eng, dname, level, linked, on):
    d, dd = dc.dictionary(dname), dev_dict(dname)
    names, inputs = zip(*dc.natural(dname))
    p = prefs(linked=linked, bck=on, cck=on, csize=on, dictid=77 if on else 0, level=level)
    enc = Encoded(eng, inputs, p, dd)
    plain = Encoded(eng, inputs, p, None)
    frames = []
    for i, data in enumerate(inputs):
        r, q, name = enc.recs[i], plain.recs[i], (dname, names[i])
        frame = enc.frame(i)
        frames.append(frame)
        assert (r.status, r.consumed, r.n_blocks, r.first_bad_block, r.flags) == (0, len(data), q.n_blocks, NONE, q.flags), name
        assert r.flags >> 12 == PATH_BATCH and frame[4] == r.flags & 0xFF == plain.frame(i)[4], name
        hs = dc.walk(frame)["blocks"][0][1] - 4 if dc.walk(frame)["blocks"] else len(frame) - 4 - (4 if on else 0)
        assert frame[:hs] == plain.frame(i)[:hs], (name, "header")
        assert enc.untouched_behind(i), name
        v = dc.model_decode(frame, d)
        assert v.ok and v.out == data and v.consumed == r.size, (name, v.why)
        check_writer_rules(frame, min(len(d), dc.KB64), name)
    dec = Decoded(eng, frames, [max(len(x), 1) for x in inputs], dd)
    for i, data in enumerate(inputs):
        assert dec.recs[i].status == 0 and dec.out(i) == data, (dname, names[i], dec.recs[i].status)
    assert sum(len(f) for f in frames) <= sum(r.size for r in plain.recs)
    if dname != "phrase" or not on: return
    # equal bytes across two calls, and between a batch of one and a batch of many
    assert Encoded(eng, inputs, p, dd).all() == enc.all()
    for i in (0, 3, 9, 14, len(inputs) - 5, len(inputs) - 1):
        one = Encoded(eng, [inputs[i]], p, dd)
        assert one.all()[0] == enc.all()[i], names[i]
    # a window one byte too small fails alone
    short = set(range(1, len(inputs), 4))
    tight = Encoded(eng, inputs, p, dd, windows=[r.size - 1 if i in short else r.size for i, r in enumerate(enc.recs)])
    for i in range(len(inputs)):
        if i in short: assert tight.recs[i].status == ST_DST_SMALL and tight.recs[i].size == 0 and tight.wins[i] == bytes([PAT]) * len(tight.wins[i]), names[i]
        else: assert tight.all()[i] == enc.all()[i], names[i]


def test_empty_dictionary_is_the_plain_call(eng, fx):
    empty = torch.zeros(0, dtype=torch.uint8, device=DEV)
    names, inputs = zip(*dc.natural("phrase"))
    for linked in (0, 1):
        p = prefs(linked=linked, bck=1, cck=1)
        assert Encoded(eng, inputs, p, empty).all() == Encoded(eng, inputs, p, None, plain_call=True).all()
    for mode in dc.MODES:
        cases = dc.fixture_frames(fx, "phrase", mode)
        frames = [c[1] for c in cases]
        wins = measure(eng, frames)
        assert Decoded(eng, frames, wins, empty).verdicts() == Decoded(eng, frames, wins, None).verdicts()


@pytest.mark.parametrize("level", (3, 9))
def test_hc_levels_take_no_dictionary(eng, level):
    inputs = [x for _, x in dc.natural("d1k")]
    lens = [len(x) for x in inputs]
    so = [0]
    for n in lens: so.append(so[-1] + n)
    p = prefs(level=level)
    do = frame_windows(lens, p, GUARD)
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(lens))
    with pytest.raises(DeviceCodecError, match="compressionLevel_invalid"):
        eng.compress_frames_async(_dev(b"".join(inputs), 16), _off(so), dst, _off(do), p, res, dictionary=dev_dict("d1k"))
    eng.stream.synchronize()
    assert bool((dst == PAT).all()) and not bool(res.any())


def test_dictionary_argument_is_checked(eng):
    src, off, res = _dev(b"x" * 64), _off([0, 64]), eng.new_results(1)
    dst = torch.zeros(256, dtype=torch.uint8, device=DEV)
    for bad in (torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.int32, device=DEV), b"abc", torch.zeros((2, 4), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            eng.compress_frames_async(src, off, dst, _off([0, 256]), prefs(), res, dictionary=bad)
        with pytest.raises(ValueError):
            eng.decompress_frames_async(src, off, dst, _off([0, 256]), res, dictionary=bad)


def test_any_alignment(eng, fx):
    """The dictionary at byte residues 0, 1 and 3, source and destination at a handful of residues: the same bytes and verdicts."""
    cases = dc.fixture_frames(fx, "d1k", "indep") + dc.fixture_frames(fx, "d1k", "linked")
    frames = [c[1] for c in cases]
    wins = measure(eng, frames)
    inputs = [x for _, x in dc.natural("d1k")]
    p = prefs(bck=1, cck=1, csize=1)
    want_d = want_e = None
    places = [(0, SRC_RES[0], DST_RES[0]), (1, SRC_RES[1], DST_RES[1]), (3, SRC_RES[3], DST_RES[2]), (1, SRC_RES[-1], DST_RES[-1]), (3, SRC_RES[7], DST_RES[3])]
    for dres, sres, tres in places:
        dd = dev_dict("d1k", dres)
        assert dd.data_ptr() % 64 == dres
        dec = Decoded(eng, frames, wins, dd, src_res=sres, dst_res=tres)
        enc = Encoded(eng, inputs, p, dd, src_res=sres, dst_res=tres)
        if want_d is None:
            check_decoded(dec, cases, wins)
            want_d, want_e = dec.verdicts(), enc.all()
        assert dec.verdicts() == want_d and enc.all() == want_e, (dres, sres, tres)


def test_ratio_against_liblz4(eng, fx):
    """A condition, not a measured constant: over the phrase dictionary's records of at most 4096 bytes the device's frames take
    at most halfway between liblz4's total with the dictionary and its total without - the encoder recovers at least half of the
    gain liblz4 measures.  (The finder seeds every fourth position of the dictionary and cuts matches at the seam.)"""
    t = fx["totals"]["phrase"]
    inputs = [x for _, x in dc.natural("phrase") if len(x) <= dc.RATIO_MAX]
    assert len(inputs) == t["records"]
    enc = Encoded(eng, inputs, prefs(), dev_dict("phrase"))
    plain = Encoded(eng, inputs, prefs(), None)
    total, without = sum(r.size for r in enc.recs), sum(r.size for r in plain.recs)
    print("device with dictionary %d, without %d; liblz4 with %d, without %d" % (total, without, t["with"], t["without"]))
    assert all(r.status == 0 for r in enc.recs)
    assert total <= (t["with"] + t["without"]) / 2, (total, t)
