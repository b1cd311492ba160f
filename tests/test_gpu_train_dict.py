"""lz4f_mi355x_dev_trainDict (Engine.train_dict_async): a dictionary trained from a batch of samples on the device.

The device equals tests/train_model.py byte for byte, and its record the model's, on the cases of tests/train_cases.py - the smallest
shapes at which each rule of the definition can go wrong, each held by tests/test_train_model_cpu.py to what it was built to show.
The dictionary and the record carry guards that must survive.  The end-to-end cases run train, create_cdict, compress and decompress on
one stream with nothing read back in between, and hold the dictionary to the fixture liblz4's sizes were minted for."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import train_cases as tc
import train_model as tm
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd._ffi import Result, TrainParams
from lz4_frame_conduit_amd.device import TRAIN_DEFAULTS, DeviceCodecError, Engine, frame_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT = 0xA5
GUARD = 64
ERR_GENERIC, ERR_SRC_TOO_LARGE = 1, 10         # LZ4F_ERROR_GENERIC, LZ4F_ERROR_srcSize_tooLarge


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def shifted(data: bytes, shift: int = 0, room: int = 16) -> torch.Tensor:
    """data in device memory, `shift` bytes past an allocation's (256-byte aligned) start, PAT around it"""
    t = torch.full((shift + len(data) + room,), PAT, dtype=torch.uint8, device=DEV)
    if data:
        t[shift:shift + len(data)].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    return t[shift:shift + len(data)]


def params_of(p: dict) -> TrainParams:
    return TrainParams(k=p["k"], d=p["d"], f=p["f"], rounds=p["rounds"])


def run_case(eng, c: tc.Case, src_shift: int = 0, dict_shift: int = 0, want_record: bool = True, want: "tm.Trained | None" = None):
    """One call held to the model, guards and all -> the dictionary's bytes"""
    want = want or tc.model(c)
    src = shifted(c.src, src_shift)
    off = torch.tensor(c.off, dtype=torch.int64, device=DEV)
    d_all = torch.full((dict_shift + GUARD + c.dict_size + GUARD,), PAT, dtype=torch.uint8, device=DEV)
    d = d_all[dict_shift + GUARD:dict_shift + GUARD + c.dict_size]
    rec_all = torch.full((96,), PAT, dtype=torch.uint8, device=DEV)
    rec = rec_all[32:64] if want_record else None
    if c.src_bytes is None:
        eng.train_dict_async(src, off, d, params_of(c.params), record=rec)
    else:                                                                      # (srcBytes smaller than the buffer: the C ABI)
        r = eng.L.lz4f_mi355x_dev_trainDict(eng.h, len(c.off) - 1, src.data_ptr(), c.src_bytes, off.data_ptr(), d.data_ptr(), c.dict_size,
                                            ctypes.byref(params_of(c.params)), rec.data_ptr() if want_record else None)
        assert r == 0
    eng.stream.synchronize()
    got_d, got_rec = d_all.cpu().numpy(), rec_all.cpu().numpy()
    lo = dict_shift + GUARD
    assert (got_d[:lo] == PAT).all() and (got_d[lo + c.dict_size:] == PAT).all(), (c.name, "bytes around the dictionary were written")
    assert (got_rec[:32] == PAT).all() and (got_rec[64:] == PAT).all(), (c.name, "bytes around the record were written")
    got = got_d[lo:lo + c.dict_size].tobytes()
    if got != want.dict:
        first = next(i for i in range(c.dict_size) if got[i] != want.dict[i])
        raise AssertionError("%s: the dictionary differs from the model's at byte %d of %d (model: %d used, log %r)" % (c.name, first, c.dict_size, want.used, want.log[:6]))
    if want_record:
        r = Result.from_buffer_copy(got_rec[32:64].tobytes())
        assert (r.size, r.consumed, r.n_blocks, r.first_bad_block, r.status, r.flags) == \
               (want.used, want.consumed, want.n_segments, want.first_bad, 0, tm.record_flags(want)), (c.name, r.size, r.consumed, r.n_blocks, r.first_bad_block, hex(r.flags))
    else:
        assert (got_rec == PAT).all()
    return got


CASES = tc.all_cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_device_equals_model(eng, c):
    """Every rule of the definition at its smallest shape (tests/train_cases.py)"""
    run_case(eng, c)


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_any_byte_address(eng, shift):
    for name in ("seams/in_segments", "tile/bytes+1"):
        c = tc.by_name(name)
        run_case(eng, c, src_shift=shift, dict_shift=16 - shift if shift != 15 else 1)
        run_case(eng, c, src_shift=0, dict_shift=shift)


def test_two_calls_give_equal_bytes_and_the_record_is_optional(eng):
    for name in ("noise_64k", "tile/three_and_a_bit", "stale/planted"):
        c = tc.by_name(name)
        assert run_case(eng, c) == run_case(eng, c, want_record=False)


def test_workspace_is_reused_across_shapes(eng):
    """A small call behind a large one (the counts and picks of the large one lie in the workspace), and a larger f behind a smaller"""
    for name in ("tile/k4096", "n/equals_d", "params/d8_f22", "dict_size/53", "n/below_d", "same_sample_x64"):
        run_case(eng, tc.by_name(name))


def test_defaults_are_the_headers(eng):
    """params=None, and a TrainParams of zeros, are TRAIN_DEFAULTS"""
    data = tc.text("defaults", 3000)
    c = tc.case("defaults", data, tc.cut(data, (500,)), 700, **TRAIN_DEFAULTS)
    want = tc.model(c)
    assert want.n_segments > 3
    for p in (None, TrainParams()):
        d = torch.full((700,), PAT, dtype=torch.uint8, device=DEV)
        eng.train_dict_async(shifted(c.src), torch.tensor(c.off, dtype=torch.int64, device=DEV), d, p)
        eng.stream.synchronize()
        assert d.cpu().numpy().tobytes() == want.dict


def test_argument_errors_enqueue_nothing(eng):
    c = tc.by_name("seams/in_segments")
    L = eng.L
    src = shifted(c.src)
    off = torch.tensor(c.off, dtype=torch.int64, device=DEV)
    d = torch.full((65536 + 64,), PAT, dtype=torch.uint8, device=DEV)
    rec = torch.full((32,), PAT, dtype=torch.uint8, device=DEV)
    n = len(c.off) - 1

    def call(e=eng.h, n=n, s=src.data_ptr(), sb=len(c.src), o=off.data_ptr(), dd=d.data_ptr(), ds=200, p=None):
        return L.lz4f_mi355x_dev_trainDict(e, n, s, sb, o, dd, ds, ctypes.byref(p) if p is not None else None, rec.data_ptr())

    def refused(r, code, word=None):
        assert L.LZ4F_isError(r) and (1 << 64) - r == code, r
        if word: assert word in L.lz4f_mi355x_last_error().decode(), L.lz4f_mi355x_last_error()

    refused(call(e=None), ERR_GENERIC)
    refused(call(s=None), ERR_GENERIC, "null pointer")
    refused(call(o=None), ERR_GENERIC, "null pointer")
    refused(call(dd=None), ERR_GENERIC, "null pointer")
    for field, bad in (("k", (3, 4097)), ("d", (5, 7, 9, 3)), ("f", (15, 23)), ("rounds", (65, 1000))):
        for v in bad:
            p = dict(k=16, d=4, f=16, rounds=4); p[field] = v
            refused(call(p=TrainParams(**p)), ERR_GENERIC, field + " ")
    refused(call(p=TrainParams(k=6, d=8)), ERR_GENERIC, "k ")                  # k below d
    refused(call(ds=65537), ERR_GENERIC, "dictSize")
    refused(call(sb=1 << 31), ERR_SRC_TOO_LARGE, "srcBytes")
    assert call(n=0) == 0 and call(ds=0) == 0 and call(n=0, s=None, o=None, dd=None) == 0 and call(ds=0, dd=None) == 0
    with pytest.raises(DeviceCodecError):
        eng.train_dict_async(src, off, d[:200], TrainParams(d=5))
    for bad in (lambda: eng.train_dict_async(src.cpu(), off, d[:200]), lambda: eng.train_dict_async(src, off.to(torch.int32), d[:200]),
                lambda: eng.train_dict_async(src, off, d), lambda: eng.train_dict_async(src, off, d[:200], params={"k": 16}),
                lambda: eng.train_dict_async(src, off, d[:200], record=rec[:31]), lambda: eng.train_dict_async(src, off[:0], d[:200])):
        with pytest.raises(ValueError):
            bad()
    eng.stream.synchronize()
    assert (d.cpu().numpy() == PAT).all() and (rec.cpu().numpy() == PAT).all(), "a refused call wrote something"
    assert call(ds=200, p=TrainParams(k=16, d=4, f=16, rounds=4)) == 0         # ... and the same arguments, valid, do run
    eng.stream.synchronize()
    assert (d[:200].cpu().numpy() != PAT).any() and (d[200:].cpu().numpy() == PAT).all()


# ---- end to end: train -> create_cdict -> compress -> decompress, one stream, nothing read back in between ----
@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_dict_sizes.json")) as f:
        return json.load(f)


def _dev(b: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(b + bytes(16), dtype=np.uint8).copy()).to(DEV)


def round_trip(eng, name: str, level: int, hc: bool):
    """-> (the trained dictionary's bytes, the frames' total with it, with the naive dictionary, with none)"""
    train, held = tm.records(name)
    src = _dev(b"".join(train))[:2048 * 1024]
    off = torch.arange(0, 2049, dtype=torch.int64, device=DEV) * 1024
    h_src = _dev(b"".join(held))
    h_off = torch.arange(0, 257, dtype=torch.int64, device=DEV) * 1024
    p = conduit.make_preferences(blockSizeID=4, blockMode=1, compressionLevel=level)
    wins = frame_windows([1024] * 256, p)
    w_off = torch.tensor(wins, dtype=torch.int64, device=DEV)
    frames = torch.zeros(wins[-1], dtype=torch.uint8, device=DEV)
    back = torch.full((256 * 1024,), PAT, dtype=torch.uint8, device=DEV)
    d = torch.full((65536,), PAT, dtype=torch.uint8, device=DEV)
    res_c, res_d = eng.new_results(256), eng.new_results(256)
    # the chain: nothing is read back before the last call is enqueued
    eng.train_dict_async(src, off, d)
    cd = eng.create_cdict(d, hc=hc)
    eng.compress_frames_async(h_src, h_off, frames, w_off, p, res_c, cdict=cd)
    eng.decompress_frames_async(frames, w_off, back, h_off, res_d, dictionary=cd)
    made, decoded = eng.frame_results(res_c), eng.frame_results(res_d)
    assert all(r.status == 0 and r.consumed == 1024 for r in made) and all(r.status == 0 and r.size == 1024 for r in decoded)
    assert back.cpu().numpy().tobytes() == b"".join(held), "a record did not come back"
    total = {"trained": sum(r.size for r in made)}
    cd.close()
    for what, dictionary in (("naive", tm.naive_dictionary(name, 65536)), ("none", None)):
        how = {}
        if dictionary is not None:
            how["cdict"] = eng.create_cdict(_dev(dictionary)[:65536], hc=hc)
        eng.compress_frames_async(h_src, h_off, frames, w_off, p, res_c, **how)
        recs = eng.frame_results(res_c)
        assert all(r.status == 0 for r in recs)
        total[what] = sum(r.size for r in recs)
        if how: how["cdict"].close()
    return d.cpu().numpy().tobytes(), total


@pytest.mark.parametrize("name", tm.CORPORA)
def test_end_to_end(eng, fx, name):
    row = [r for r in fx["rows"] if r["corpus"] == name and r["dict_size"] == 65536][0]
    got, total = round_trip(eng, name, 0, False)
    assert tm.sha(got) == row["sha256"], "the device's dictionary is not the one the fixture's sizes were minted for"
    print(name, total, "liblz4:", {k: row[k] for k in ("trained", "naive", "none")})
    assert total["trained"] < total["naive"] and total["trained"] < total["none"], total


def test_end_to_end_level3_hc(eng, fx):
    row = [r for r in fx["rows"] if r["corpus"] == "uniform" and r["dict_size"] == 65536][0]
    got, total = round_trip(eng, "uniform", 3, True)
    assert tm.sha(got) == row["sha256"]
    print("uniform, level 3", total)
    assert total["trained"] < total["none"], total
