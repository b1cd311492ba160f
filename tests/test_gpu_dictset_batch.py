"""A set of dictionaries for the batch calls, one chosen per frame: lz4f_mi355x_dev_createDictSet, _resolveDictIDs,
_compressFrames_usingDictSet, _decompressFrames_usingDictSet (Engine.create_dictset, compress_frames_async / decompress_frames_async
(..., dictset=, slots=), resolve_dict_ids_async).

The yardstick throughout is the one-dictionary call in a batch of one on the same engine - lz4f_mi355x_dev_compressFrames_usingCDict
with the frame's member and that member's ID in the preferences, lz4f_mi355x_dev_decompressFrames_usingDict with the member's bytes,
the plain calls for LZ4F_MI355X_DICT_NONE - existing code, held to liblz4 and to the dictionary model by tests/test_gpu_dict_batch.py,
test_gpu_cdict_batch.py and test_gpu_cdict_hc.py.  A frame's bytes, its record and its whole window must be that call's: no
tolerance.  The twins run on the batch's own buffers (span i and window i of a second, pattern-filled destination), all of them
enqueued before one read-back."""
import numpy as np
import pytest
import torch

import dict_cases as dc
import dictset_cases as ds
from alignment_cases import carve, intact
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd.device import (DICT_NONE, DICT_UNKNOWN, PATH_DICT_UNKNOWN, DeviceCodecError, DictSet, Engine, Result, frame_windows,
                                          peek_pack_directory)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 192
PAT = 0xA5
RB = 32                                             # a result record's bytes
UNKNOWN_REC = (ds.ST_GENERIC, 0, 0, 0, 0xFFFFFFFF, (ds.PATH_BATCH | ds.PATH_DICT_UNKNOWN) << 12)
assert (DICT_NONE, DICT_UNKNOWN, PATH_DICT_UNKNOWN) == (ds.NONE, ds.UNKNOWN, ds.PATH_DICT_UNKNOWN)


def _dev(b, extra: int = 0) -> torch.Tensor:
    a = np.frombuffer(bytes(b) + b"\0" * extra, dtype=np.uint8) if len(b) + extra else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a.copy()).to(DEV)


def _off(v) -> torch.Tensor:
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


def _slots(v, misaligned: bool = False) -> torch.Tensor:
    """Slots in device memory; misaligned: at a 4-byte address that is not 8-byte aligned."""
    a = ds.slots_array(v)
    if not misaligned: return torch.from_numpy(a.copy()).to(DEV)
    t = torch.zeros(len(a) + 1, dtype=torch.int32, device=DEV)[1:]
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 8 == 4 and t.is_contiguous()
    return t


def dev_bytes(b: bytes, res: int = 0) -> torch.Tensor:
    view, _, _ = carve(len(b), res, device=DEV)
    if len(b): view.copy_(_dev(b))
    return view


class World:
    """An engine, a plain and a hash-chain CDict of every dictionary, and the two sets of them (the empty member: an empty CDict in
    the plain set, NULL in the hash-chain one)."""

    def __init__(self, dict_res: int = 0):
        self.eng = Engine(0)
        self.cd, self.hc = {}, {}
        for name in ds.MEMBERS:
            if name is None: continue
            d = dev_bytes(dc.dictionary(name), dict_res)
            self.cd[name], self.hc[name] = self.eng.create_cdict(d), self.eng.create_cdict(d, hc=True)
        self.empty = self.eng.create_cdict(torch.zeros(0, dtype=torch.uint8, device=DEV))
        self.set = self.eng.create_dictset([self.cd[m] if m else self.empty for m in ds.MEMBERS], ds.IDS)
        self.set_hc = self.eng.create_dictset([self.hc[m] if m else None for m in ds.MEMBERS], ds.IDS)

    def of(self, level: int):
        return (self.set_hc, self.hc) if level >= 3 else (self.set, self.cd)

    def member(self, slot: int, level: int = 0):
        """The CDict a slot stands for (DICT_NONE and the empty member: None)."""
        return None if slot == ds.NONE or ds.MEMBERS[slot] is None else self.of(level)[1][ds.MEMBERS[slot]]

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def w():
    x = World()
    yield x
    x.close()


@pytest.fixture(scope="module")
def fx():
    f = dc.load_fixture()
    dc.check_sha(f)
    return f


def prefs(linked=0, on=0, level=0, dict_id=None, bsid=4):
    return conduit.make_preferences(blockSizeID=bsid, blockMode=0 if linked else 1, blockChecksum=on, contentChecksum=on, contentSize=1 if on else 0,
                                    dictID=(77 if on else 0) if dict_id is None else dict_id, compressionLevel=level)


def rec_tuple(r):
    return (r.status, r.size, r.consumed, r.n_blocks, r.first_bad_block, r.flags)


def records(eng, res, n):
    eng.stream.synchronize()
    raw = res.cpu().numpy().tobytes()
    return [rec_tuple(Result.from_buffer_copy(raw, k * RB)) for k in range(n)]


class Batch:
    """The buffers of one batch: spans back to back in `src` (at byte residue src_res), windows back to back in a pattern-filled
    destination (at dst_res) - and a second destination and record array of the same layout for the batch-of-one twins."""

    def __init__(self, eng, spans, windows, src_res=0, dst_res=0):
        self.eng, self.n = eng, len(spans)
        self.so, self.do = [0], [0]
        for s, wn in zip(spans, windows):
            self.so.append(self.so[-1] + len(s)); self.do.append(self.do[-1] + wn)
        self.src, _, _ = carve(self.so[-1] + 16, src_res, device=DEV)
        self.src.copy_(_dev(b"".join(spans), 16))
        self.so_t, self.do_t = _off(self.so), _off(self.do)
        self.dst_res = dst_res

    def fresh(self):
        dst, g0, g1 = carve(max(self.do[-1], 1), self.dst_res, device=DEV)
        return dst, (g0, g1), self.eng.new_results(self.n)

    def read(self, dst, guards, res, idx=None):
        """-> {i: (record, the window's bytes)}"""
        recs = records(self.eng, res, self.n)
        out = dst.cpu().numpy().tobytes()
        assert intact(*guards)
        return {i: (recs[i], out[self.do[i]:self.do[i + 1]]) for i in (range(self.n) if idx is None else idx)}

    def one(self, i):
        """Frame i's arguments for a batch of one on these buffers."""
        return self.so_t[i:i + 2], self.do_t[i:i + 2]


def compress_set(w, inputs, p, slots, level=0, windows=None, src_res=0, dst_res=0, slot_misaligned=False):
    lens = [len(x) for x in inputs]
    if windows is None:
        bound = frame_windows(lens, prefs(on=1, dict_id=1), GUARD)                     # (room for every header field whatever the frame's ID is)
        windows = [bound[i + 1] - bound[i] for i in range(len(lens))]
    b = Batch(w.eng, inputs, windows, src_res, dst_res)
    dst, guards, res = b.fresh()
    w.eng.compress_frames_async(b.src, b.so_t, dst, b.do_t, p, res, dictset=w.of(level)[0], slots=_slots(slots, slot_misaligned))
    return b, b.read(dst, guards, res)


def compress_twins(w, b, idx, p, slots, level=0):
    """The batch-of-one calls of the frames `idx`: _usingCDict with the member and its ID, the plain call for DICT_NONE."""
    dst, guards, res = b.fresh()
    for i in idx:
        pi = prefs(linked=1 - p.frameInfo.blockMode, on=p.frameInfo.contentChecksumFlag, level=p.compressionLevel, bsid=p.frameInfo.blockSizeID,
                   dict_id=ds.member_id(slots[i], p.frameInfo.dictID))
        so, do = b.one(i)
        w.eng.compress_frames_async(b.src, so, dst, do, pi, res[i * RB:(i + 1) * RB], cdict=w.member(slots[i], level))
    return b.read(dst, guards, res, idx)


def assert_same(got, want, what):
    for i in want:
        assert got[i][0] == want[i][0], (what, i, got[i][0], want[i][0])
        assert got[i][1] == want[i][1], (what, i, "window bytes differ")


def decompress_set(w, frames, windows, slots, level=0, **place):
    b = Batch(w.eng, frames, windows, place.get("src_res", 0), place.get("dst_res", 0))
    dst, guards, res = b.fresh()
    w.eng.decompress_frames_async(b.src, b.so_t, dst, b.do_t, res, dictset=w.of(level)[0],
                                  slots=None if slots is None else _slots(slots, place.get("slot_misaligned", False)))
    return b, b.read(dst, guards, res)


def decompress_twins(w, b, idx, slots, level=0):
    """The batch-of-one calls of the frames `idx`: _usingDict with the member's bytes (the CDict's copy), the plain call without."""
    dst, guards, res = b.fresh()
    for i in idx:
        so, do = b.one(i)
        w.eng.decompress_frames_async(b.src, so, dst, do, res[i * RB:(i + 1) * RB], dictionary=w.member(slots[i], level))
    return b.read(dst, guards, res, idx)


def measure(eng, frames) -> "list[int]":
    so = [0]
    for f in frames: so.append(so[-1] + len(f))
    do = torch.zeros(len(frames) + 1, dtype=torch.int64, device=DEV)
    eng.measure_frames_async(_dev(b"".join(frames), 16), _off(so), eng.new_results(len(frames)), do)
    eng.stream.synchronize()
    v = do.cpu().tolist()
    return [v[i + 1] - v[i] for i in range(len(frames))]


def frames_of(got, n):
    return [got[i][1][:got[i][0][1]] for i in range(n)]


# ---- 1: equal frames, compress ----
@pytest.mark.parametrize("on", (0, 1))
@pytest.mark.parametrize("linked", (0, 1))
@pytest.mark.parametrize("level", (0, 2, 3, 9))
def test_equal_frames_compress(w, level, linked, on):
    inputs = [x for _, x in ds.compress_inputs()]
    slots = ds.slot_cycle(len(inputs), shift=level + linked)
    assert set(slots) == set(range(len(ds.MEMBERS))) | {ds.NONE}
    p = prefs(linked, on, level)
    b, got = compress_set(w, inputs, p, slots, level)
    want = compress_twins(w, b, range(len(inputs)), p, slots, level)
    assert all(v[0][0] == 0 for v in want.values())
    assert_same(got, want, (level, linked, on))
    big = [i for i, x in enumerate(inputs) if len(x) >= 65535]
    assert len({slots[i] for i in big}) >= 3 and any(got[i][0][3] > 1 for i in big)       # (several blocks, different members)
    # the header's dictID is the member's; ID 0 writes no field; a DICT_NONE frame carries the call's
    for i, s in enumerate(slots):
        f = got[i][1]
        at, want_id = ds.dict_id_at(f), ds.member_id(s, p.frameInfo.dictID)
        assert (at is None) == (want_id == 0), (i, s)
        if at is not None: assert int.from_bytes(f[at:at + 4], "little") == want_id, (i, s)


# ---- 2: a workgroup crosses dictionaries ----
@pytest.mark.parametrize("level, n, grid", ((0, 16500, 16384), (3, 2100, 2048)))
def test_a_workgroup_crosses_dictionaries(w, level, n, grid):
    """More frames than the finder has workgroups, so that a workgroup takes chunk i and then chunk i + grid - of another member."""
    slots = ds.crossing_slots(n, 2048, 16384)
    inputs = ds.crossing_records(n, slots, grid)
    assert n > grid and all(64 <= len(x) <= 200 for x in inputs)
    p = prefs(0, 1, level, dict_id=0)
    b, got = compress_set(w, inputs, p, slots, level)
    r = dc.rng_of("crossing/sample")
    # (the first and last 64, a seeded sample of 256, and every frame behind the grid's end: a workgroup's second chunk)
    idx = sorted(set(range(64)) | set(range(n - 64, n)) | {int(k) for k in r.integers(0, n, 256)} | set(range(grid, n)))
    want = compress_twins(w, b, idx, p, slots, level)
    assert all(v[0][0] == 0 for v in want.values())
    assert_same(got, want, level)
    # and all of them decode, each with its member, to the inputs
    frames = frames_of(got, n)
    _, dec = decompress_set(w, frames, [len(x) for x in inputs], slots, level)
    bad = [i for i in range(n) if dec[i][0][0] != 0 or dec[i][1] != inputs[i]]
    assert not bad, bad[:10]


# ---- 3: equal results, decode, slots given ----
def test_equal_results_decode(w, fx):
    cases = ds.decode_cases(fx)
    frames, slots = [c[1] for c in cases], [c[3] for c in cases]
    wins = measure(w.eng, frames)
    b, got = decompress_set(w, frames, wins, slots)
    want = decompress_twins(w, b, range(len(frames)), slots)
    assert_same(got, want, "fixture")
    ok = 0
    for i, (name, _, exp, _) in enumerate(cases):
        rec, win = got[i]
        if exp is None:
            assert rec[0] != 0, name                                                  # (liblz4 rejects it; the neighbours stand: assert_same)
        else:
            assert rec[0] == 0 and rec[1] == len(exp) and win[:rec[1]] == exp, (name, rec)
            ok += 1
    assert ok >= 150 and len(frames) - ok >= 6


# ---- 4: by header ----
@pytest.mark.parametrize("level", (0, 3))
def test_by_header(w, level):
    inputs = [x for _, x in ds.compress_inputs()]
    n = len(inputs)
    slots = ds.slot_cycle(n, shift=1)
    assert slots[[k for k, _ in ds.compress_inputs()].index("d1k/tail")] == ds.IDS.index(0)      # (a record that leans on the ID-0 member)
    p = prefs(level % 2, 1, level, dict_id=0)                                          # (DICT_NONE frames carry no field)
    _, enc = compress_set(w, inputs, p, slots, level)
    assert all(enc[i][0][0] == 0 for i in range(n))
    frames = frames_of(enc, n)
    zero = ds.IDS.index(0)
    expect = [ds.NONE if s == zero else s for s in slots]
    assert expect != slots
    b, got = decompress_set(w, frames, [len(x) for x in inputs], None, level)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    w.eng.resolve_dict_ids_async(b.src, b.so_t, w.of(level)[0], out)
    w.eng.stream.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == expect
    # every frame is what the batch-of-one call gives it with the member its header names
    assert_same(got, decompress_twins(w, b, range(n), expect, level), "by header")
    for i in range(n):
        if slots[i] != zero:
            assert got[i][0][0] == 0 and got[i][1] == inputs[i], (i, got[i][0])
    # the ID-0 member's frames carry no field: they decode as the plain call decodes them, whatever that makes of them
    dst, guards, res = b.fresh()
    w.eng.decompress_frames_async(b.src, b.so_t, dst, b.do_t, res)
    plain = b.read(dst, guards, res)
    mine = [i for i in range(n) if slots[i] == zero]
    assert len(mine) >= 5
    for i in mine: assert got[i] == plain[i], i
    assert any(got[i][0][0] != 0 for i in mine)                                        # (some of them did use their dictionary)


def test_forged_dict_ids(w):
    x = dc.natural("phrase")[12][1]
    assert len(x) == 300
    b0 = Batch(w.eng, [x, x], frame_windows([len(x)] * 2, prefs(on=1, dict_id=1), GUARD)[1:2] * 2)
    dst, guards, res = b0.fresh()
    w.eng.compress_frames_async(b0.src, b0.so_t, dst, b0.do_t, prefs(on=1, dict_id=5), res, cdict=w.cd["d1k"])
    made = b0.read(dst, guards, res)
    f = made[0][1][:made[0][0][1]]
    assert made[0][0][0] == 0 and ds.dict_id_at(f) is not None
    absent, zero = ds.patch_dict_id(f, ds.ABSENT_ID), ds.patch_dict_id(f, 0)
    assert ds.dict_id_at(zero) is not None                                             # (the field is there and holds the literal value 0)
    frames = [absent, zero, f]                                                         # (5 is no member's ID either)
    b, got = decompress_set(w, frames, [len(x) + 7] * 3, None)
    out = torch.zeros(3, dtype=torch.int32, device=DEV)
    w.eng.resolve_dict_ids_async(b.src, b.so_t, w.set, out)
    w.eng.stream.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == [ds.UNKNOWN, ds.slot_of("d1k"), ds.UNKNOWN]
    for i in (0, 2):
        assert got[i][0] == UNKNOWN_REC and got[i][1] == bytes([PAT]) * (len(x) + 7), (i, got[i][0])
    assert got[1][0][:2] == (0, len(x)) and got[1][1][:len(x)] == x


# ---- 5: the wrong member is caught only by the checksum ----
def test_wrong_member_is_caught_only_by_the_checksum(w):
    inputs = [x for name, x in dc.natural("phrase") if name in ("n300", "n1000", "n4096", "slice", "tail")]
    n = len(inputs)
    right = [ds.slot_of("phrase")] * n
    _, enc = compress_set(w, inputs, prefs(0, 1), right)
    frames = frames_of(enc, n)
    ST_CONTENTCK = 18
    # d1k: 1 KiB where the frames reach 64 KiB back - an offset that does not fit is a block error; big: every offset fits, the bytes
    # are wrong, and only the content checksum says so
    for name, only in (("d1k", None), ("big", ST_CONTENTCK)):
        wrong = [ds.slot_of(name)] * n
        b, got = decompress_set(w, frames, [len(x) for x in inputs], wrong)
        assert_same(got, decompress_twins(w, b, range(n), wrong), name)
        st = [got[i][0][0] for i in range(n)]
        assert all(v != 0 for v in st) and (only is None or st == [only] * n), (name, [got[i][0] for i in range(n)])


# ---- 6: forged slots ----
def test_forged_slots(w):
    count = len(ds.MEMBERS)
    forged = {3: count, 8: count + 1, 13: 0x7FFFFFFF, 21: ds.UNKNOWN}
    inputs = [x for _, x in ds.compress_inputs()][:30]
    n = len(inputs)
    good = ds.slot_cycle(n)
    slots = [forged.get(i, s) for i, s in enumerate(good)]
    p = prefs(0, 1)
    b, was = compress_set(w, inputs, p, good)
    _, got = compress_set(w, inputs, p, slots)
    for i in range(n):
        if i in forged: assert got[i][0] == UNKNOWN_REC and got[i][1] == bytes([PAT]) * len(got[i][1]), (i, got[i][0])
        else: assert got[i] == was[i], i
    frames = frames_of(was, n)
    wins = [len(x) + 5 for x in inputs]
    _, dwas = decompress_set(w, frames, wins, good)
    _, dgot = decompress_set(w, frames, wins, slots)
    for i in range(n):
        if i in forged: assert dgot[i][0] == UNKNOWN_REC and dgot[i][1] == bytes([PAT]) * wins[i], (i, dgot[i][0])
        else: assert dgot[i] == dwas[i] and dgot[i][0][0] == 0 and dgot[i][1][:len(inputs[i])] == inputs[i], i


# ---- 7: alignment ----
@pytest.mark.parametrize("res", (1, 3))
def test_alignment(w, res):
    inputs = [x for _, x in ds.compress_inputs()]
    inputs = inputs[:24] + inputs[-12:]
    n = len(inputs)
    slots = ds.slot_cycle(n, shift=res)
    w2 = World(dict_res=res)                                                           # (the members made from dictionaries at this residue)
    try:
        for level, linked in ((0, 1), (3, 0)):
            p = prefs(linked, 1, level)
            _, want = compress_set(w, inputs, p, slots, level)
            _, got = compress_set(w2, inputs, p, slots, level, src_res=res, dst_res=res, slot_misaligned=True)
            assert got == want, (res, level)
            frames, wins = frames_of(want, n), [len(x) for x in inputs]
            _, dwant = decompress_set(w, frames, wins, slots, level)
            _, dgot = decompress_set(w2, frames, wins, slots, level, src_res=res, dst_res=res, slot_misaligned=True)
            assert dgot == dwant and all(dgot[i][0][0] == 0 and dgot[i][1] == inputs[i] for i in range(n)), (res, level)
    finally:
        w2.close()


# ---- 8: the level rule and the arguments ----
def _one_call(eng, p, n=6, **how):
    inputs = [x for _, x in dc.natural("d1k")][:n]
    lens = [len(x) for x in inputs]
    so = [0]
    for k in lens: so.append(so[-1] + k)
    do = frame_windows(lens, prefs(on=1, dict_id=1), GUARD)
    dst = torch.full((do[-1],), PAT, dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(lens))
    return (lambda e: e.compress_frames_async(_dev(b"".join(inputs), 16), _off(so), dst, _off(do), p, res, **how)), dst, res


def test_level_rule(w):
    """One non-empty member without the hash-chain digest refuses levels 3-12 for the whole call, whatever the slots say."""
    mixed = w.eng.create_dictset([w.hc["phrase"], w.cd["d1k"], None], (1, 2, 3))
    try:
        for level in (3, 9):
            call, dst, res = _one_call(w.eng, prefs(level=level), dictset=mixed, slots=_slots([0, 0, 2, ds.NONE, 0, 2]))
            with pytest.raises(DeviceCodecError, match="compressionLevel_invalid"):
                call(w.eng)
            w.eng.stream.synchronize()
            assert bool((dst == PAT).all()) and not bool(res.any())
        call, dst, res = _one_call(w.eng, prefs(level=2), dictset=mixed, slots=_slots([0, 1, 2, ds.NONE, 0, 1]))
        call(w.eng)
        assert all(r[0] == 0 for r in records(w.eng, res, 6))
        # members of 1-3 bytes and empty ones do not count: the finder ignores them
        with w.eng.create_dictset([w.hc["phrase"], w.hc["d3"], w.empty], (1, 2, 3)) as fine:
            call, dst, res = _one_call(w.eng, prefs(level=3), dictset=fine, slots=_slots([0, 1, 2, ds.NONE, 0, 1]))
            call(w.eng)
            assert all(r[0] == 0 for r in records(w.eng, res, 6))
    finally:
        mixed.close()


def test_call_errors(w):
    other = Engine(0)
    try:
        foreign = other.create_cdict(dev_bytes(dc.dictionary("d1k")))
        with pytest.raises(DeviceCodecError, match="another engine"):
            w.eng.create_dictset([w.cd["d1k"], foreign], (1, 2))
        with pytest.raises(DeviceCodecError, match="duplicate dictID 7"):
            w.eng.create_dictset([w.cd["d1k"], None, w.cd["phrase"]], (7, 8, 7))
        # a set of another engine
        theirs = other.create_dictset([foreign], (1,))
        call, dst, res = _one_call(w.eng, prefs(), dictset=theirs, slots=_slots([0] * 6))
        with pytest.raises(DeviceCodecError, match="another engine"):
            call(w.eng)
        torch.cuda.synchronize()
        assert bool((dst == PAT).all()) and not bool(res.any())
    finally:
        other.close()
    assert foreign.h is None and theirs.h is None
    # a NULL set, through the C ABI
    L, e = w.eng.L, w.eng
    one = torch.zeros(64, dtype=torch.uint8, device=DEV)
    off, slot, res = _off([0, 8]), _slots([ds.NONE]), e.new_results(1)
    for r in (L.lz4f_mi355x_dev_compressFrames_usingDictSet(e.h, 1, one.data_ptr(), 8, off.data_ptr(), one.data_ptr(), 64, off.data_ptr(), None, res.data_ptr(), None, slot.data_ptr()),
              L.lz4f_mi355x_dev_decompressFrames_usingDictSet(e.h, 1, one.data_ptr(), 8, off.data_ptr(), one.data_ptr(), 64, off.data_ptr(), res.data_ptr(), None, None),
              L.lz4f_mi355x_dev_resolveDictIDs(e.h, 1, one.data_ptr(), 8, off.data_ptr(), None, slot.data_ptr()),
              L.lz4f_mi355x_dev_compressFrames_usingDictSet(e.h, 1, one.data_ptr(), 8, off.data_ptr(), one.data_ptr(), 64, off.data_ptr(), None, res.data_ptr(), w.set.h, None)):
        assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"
    # n_frames == 0 returns 0, whatever else is there
    assert L.lz4f_mi355x_dev_compressFrames_usingDictSet(e.h, 0, None, 0, None, None, 0, None, None, None, w.set.h, None) == 0
    assert L.lz4f_mi355x_dev_decompressFrames_usingDictSet(e.h, 0, None, 0, None, None, 0, None, None, w.set.h, None) == 0
    assert L.lz4f_mi355x_dev_resolveDictIDs(e.h, 0, None, 0, None, w.set.h, None) == 0
    e.stream.synchronize()
    assert not bool(res.any())


def test_python_checks_its_arguments(w):
    good = _slots([0] * 6)
    for how in (dict(dictset=w.set, slots=good, cdict=w.cd["d1k"]), dict(dictset=w.set, slots=good, dictionary=dev_bytes(b"abcd")), dict(dictset=w.set),
                dict(slots=good), dict(dictset=w.set, slots=_slots([0] * 5)), dict(dictset=w.set, slots=torch.zeros(6, dtype=torch.int64, device=DEV)),
                dict(dictset=w.set, slots=torch.zeros(6, dtype=torch.int32)), dict(dictset=w.set, slots=torch.zeros(12, dtype=torch.int32, device=DEV)[::2]),
                dict(dictset=w.cd["d1k"], slots=good)):
        call, dst, res = _one_call(w.eng, prefs(), **how)
        with pytest.raises(ValueError):
            call(w.eng)
    with pytest.raises(ValueError):
        w.eng.create_dictset([w.cd["d1k"]], (1, 2))
    with pytest.raises(ValueError):
        w.eng.create_dictset([w.cd["d1k"]], (1 << 32,))
    with pytest.raises(ValueError):
        w.eng.create_dictset([b"abc"], (1,))


def test_empty_set_is_the_plain_call_and_a_set_is_not_consumed(w):
    inputs = [x for _, x in ds.compress_inputs()][:20]
    n = len(inputs)
    lens = [len(x) for x in inputs]
    with w.eng.create_dictset([], []) as empty:
        assert len(empty) == 0 and len(w.set) == len(ds.MEMBERS)
        p = prefs(1, 1)
        bound = frame_windows(lens, prefs(on=1, dict_id=1), GUARD)
        b = Batch(w.eng, inputs, [bound[i + 1] - bound[i] for i in range(n)])
        dst, guards, res = b.fresh()
        w.eng.compress_frames_async(b.src, b.so_t, dst, b.do_t, p, res)
        plain = b.read(dst, guards, res)
        dst, guards, res = b.fresh()
        w.eng.compress_frames_async(b.src, b.so_t, dst, b.do_t, p, res, dictset=empty, slots=_slots([ds.NONE] * n))
        assert b.read(dst, guards, res) == plain
        # in an empty set every index is no member
        dst, guards, res = b.fresh()
        w.eng.compress_frames_async(b.src, b.so_t, dst, b.do_t, p, res, dictset=empty, slots=_slots([0] * n))
        assert all(v[0] == UNKNOWN_REC for v in b.read(dst, guards, res).values())
    slots = ds.slot_cycle(n)
    _, first = compress_set(w, inputs, prefs(0, 1), slots)
    _, second = compress_set(w, inputs, prefs(0, 1), slots)
    assert first == second and all(v[0][0] == 0 for v in first.values())


def test_close_order():
    e = Engine(0)
    c1, c2 = e.create_cdict(dev_bytes(dc.dictionary("d1k"))), e.create_cdict(dev_bytes(dc.dictionary("d3")), hc=True)
    s = e.create_dictset([c1, None, c2], (5, 6, 7))
    assert isinstance(s, DictSet) and len(s) == 3
    s.close(); s.close()
    assert s.h is None and len(s) == 0
    with pytest.raises(ValueError):
        _one_call(e, prefs(), dictset=s, slots=_slots([0] * 6))[0](e)
    # a member closed first takes the sets that borrow it with it; the engine closes what its caller forgot, sets before CDicts
    s2, s3 = e.create_dictset([c1, c2], (1, 2)), e.create_dictset([c2], (1,))
    c1.close()
    assert s2.h is None and s3.h is not None and c2.h is not None
    e.close()
    assert s3.h is None and c2.h is None
    s3.close(); c2.close(); e.close()


# ---- 9: the whole chain on one stream ----
def test_the_whole_chain_on_one_stream(w):
    """compress with the set -> pack with a directory -> read the directory -> measure -> decode by the headers' IDs: no host read
    between the calls."""
    inputs = [x for _, x in ds.compress_inputs()]
    n = len(inputs)
    zero = ds.IDS.index(0)
    slots = [s if s != zero else ds.slot_of("phrase") for s in ds.slot_cycle(n, shift=2)]    # (ID 0 says nothing in a header)
    lens = [len(x) for x in inputs]
    eng = w.eng
    p = prefs(1, 1, dict_id=0)
    bound = frame_windows(lens, prefs(on=1, dict_id=1), GUARD)
    b = Batch(eng, inputs, [bound[i + 1] - bound[i] for i in range(n)])
    win, _, res = b.fresh()
    pack = torch.full((bound[-1] + 24 + 4 * n,), PAT, dtype=torch.uint8, device=DEV)
    pack_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    src_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    dst_off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    res2 = eng.new_results(n)
    total = sum(lens)
    out = torch.full((2 * total + 65536,), PAT, dtype=torch.uint8, device=DEV)             # (measureFrames' windows: a frame's size at the least)
    eng.compress_frames_async(b.src, b.so_t, win, b.do_t, p, res, dictset=w.set, slots=_slots(slots))
    eng.pack_frames_async(win, b.do_t, res, pack, pack_off, directory=True)
    eng.read_pack_directory_async(pack, n, src_off)
    eng.measure_frames_async(pack, src_off, res2, dst_off)
    eng.decompress_frames_async(pack, src_off, out, dst_off, res2, dictset=w.set, slots=None)
    recs = records(eng, res2, n)                                                       # the one read-back
    assert all(r[0] == 0 for r in recs), [r for r in recs if r[0]][:3]
    do = dst_off.cpu().tolist()
    got = out.cpu().numpy().tobytes()
    assert do[n] <= out.numel() and [r[1] for r in recs] == lens
    for i, x in enumerate(inputs): assert got[do[i]:do[i] + len(x)] == x, i
    assert got[do[n]:] == bytes([PAT]) * (out.numel() - do[n])
    d, nn, fb = peek_pack_directory(pack[:24].cpu().numpy().tobytes())
    assert nn == n and d == 24 + 4 * n
