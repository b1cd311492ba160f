"""Levels 3-12 (csrc/encode_hc.cuh) held to the sequential model of tests/hc_model.py, byte for byte, on the cases of
tests/hc_choice_cases.py: which candidate wins, when the walk gives up, when the lazy parse moves on, how far a match is pulled
back - at the finder's seams (batches of 960 positions, the parse's 64-lane window, the chain ring's wrap, the 16-bit head, the 258-
and 255-byte caps, the 65535-byte reach, the dictionary seam).

Every case goes through compress_async (k_find_matches_hc) and, alone in its batch, through compress_frames_async (k_bc_find_hc);
the cases with a dictionary through the prepared HC dictionary of the batch call.  The finder is a function of its input, so there
is no tolerance and no list of exemptions: the frame's matches, its stored blocks and its size are the model's.
tests/test_hc_model_cpu.py holds the model itself to a search without hash or chain and to the block format."""
import numpy as np
import pytest
import torch

import dict_cases as dc
import hc_choice_cases as cc
import lz4_writer_rules as wr
import oracle
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd.device import Engine, frame_windows
from lz4_index import Parsed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENG = {}


def engine(attempts) -> Engine:
    """An engine made with LZ4F_MI355X_HC_ATTEMPTS = attempts (None: unset; the engine reads the switch when it is made)."""
    if attempts not in _ENG:
        with pytest.MonkeyPatch.context() as mp:
            if attempts is None: mp.delenv("LZ4F_MI355X_HC_ATTEMPTS", raising=False)
            else: mp.setenv("LZ4F_MI355X_HC_ATTEMPTS", str(attempts))
            _ENG[attempts] = Engine(0)
    return _ENG[attempts]


def prefs(fr: str, level: int):
    f = cc.FRAMINGS[fr]
    return conduit.make_preferences(blockSizeID=f["bsid"], blockMode=0 if f["linked"] else 1, compressionLevel=level)


def _dev(b: bytes, extra: int = 16) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b) + bytes(extra), dtype=np.uint8).copy()).to(DEV)


def single(eng, data: bytes, p) -> bytes:
    src = _dev(data)
    dst = torch.zeros(eng.frame_bound(len(data), p), dtype=torch.uint8, device=DEV)
    eng.compress_async(src[:len(data)], dst, p)
    r = eng.result()
    return dst[:r.size].cpu().numpy().tobytes()


def batch_of_one(eng, data: bytes, p, cdict=None) -> bytes:
    do = frame_windows([len(data)], p, 0)
    dst = torch.zeros(do[-1], dtype=torch.uint8, device=DEV)
    res = eng.new_results(1)
    off = lambda v: torch.tensor(list(v), dtype=torch.int64, device=DEV)
    eng.compress_frames_async(_dev(data), off([0, len(data)]), dst, off(do), p, res, **(dict(cdict=cdict) if cdict is not None else {}))
    r = eng.frame_results(res)[0]
    assert r.status == 0, r.status
    return dst[:r.size].cpu().numpy().tobytes()


def device_decode(eng, frame: bytes, n: int, cdict=None) -> bytes:
    if cdict is None:
        back = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
        eng.decompress_frame_async(_dev(frame, 0), len(frame), back)
        r = eng.result()
        assert r.size == n, (r.size, n)
        return back[:n].cpu().numpy().tobytes()
    dst = torch.zeros(max(n, 1), dtype=torch.uint8, device=DEV)
    res = eng.new_results(1)
    off = lambda v: torch.tensor(list(v), dtype=torch.int64, device=DEV)
    eng.decompress_frames_async(_dev(frame), off([0, len(frame)]), dst, off([0, max(n, 1)]), res, dictionary=cdict)
    r = eng.frame_results(res)[0]
    assert (r.status, r.size) == (0, n), (r.status, r.size, n)
    return dst[:n].cpu().numpy().tobytes()


def first_difference(got, want, fr: str) -> str:
    """The first row that differs with the two rows on either side, and where it lies among the finder's seams."""
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    row = (want[k] if k < len(want) else got[k]) if max(len(got), len(want)) > k else None
    where = ""
    if row is not None:
        f = cc.FRAMINGS[fr]
        pos = row[0]
        b0 = pos // f["bs"] * f["bs"]
        c0 = b0 + (pos - b0) // cc.CHUNK * cc.CHUNK
        low = 0 if f["linked"] else b0
        w = pos - (c0 - min(cc.CHUNK, c0 - low))                                   # its position in the chunk's window (no dictionary)
        where = "; input position %d = window position %d of chunk %d: mod 960 = %d, mod 64 = %d, %s the ring's wrap" % (
            pos, w, pos // cc.CHUNK, w % cc.HC_T, w % 64, "beyond" if w >= cc.RING else "before")
    return "%d rows, the model has %d; first difference at row %d (position, length, offset, literals): the frame %s, the model %s%s" % (
        len(got), len(want), k, got[max(k - 2, 0):k + 3], want[max(k - 2, 0):k + 3], where)


def check(c, fr: str, level: int):
    f = cc.FRAMINGS[fr]
    eng = engine(c.attempts)
    p = prefs(fr, level)
    data, d = c.data, c.dictionary
    what = (c.name, fr, level)
    P = c.parse(fr, level)
    if d is None:
        frame = single(eng, data, p)
        assert batch_of_one(eng, data, p) == frame, what
        cdict = None
    else:
        with eng.create_cdict(_dev(d, 0) if d else torch.zeros(0, dtype=torch.uint8, device=DEV), hc=True) as cdict:
            frame = batch_of_one(eng, data, p, cdict)
            assert batch_of_one(eng, data, p, cdict) == frame, what
            back = device_decode(eng, frame, len(data), cdict)
    parsed = Parsed(frame)
    got, want = wr.matches(frame, parsed).tolist(), P.rows.tolist()
    if got != want: pytest.fail("%s: %s" % (what, first_difference(got, want, fr)))          # (the whole message, not pytest's excerpt)
    assert [k for k, B in enumerate(parsed.blocks) if B["stored"]] == P.stored, what
    assert len(frame) == P.frame_size(), (what, len(frame), P.frame_size())
    tail = len(d[-65536:]) if d is not None and len(d) >= 4 else 0
    assert wr.audit(frame, data, dict(bsid=f["bsid"], linked=f["linked"], bck=False, cck=False), parsed, dict_len=tail) == [], what
    if d is None:
        out, used = oracle.decompress_frame(frame, cap=len(data) + 64)
        assert out == data and used == len(frame), what
        back = device_decode(eng, frame, len(data))
    else:
        v = dc.model_decode(frame, d)
        assert v.ok and v.out == data and v.consumed == len(frame), (what, v.why)
    assert back == data, what


PAIRS = [(fam, fr) for fam in cc.FAMILIES if fam != "text" for fr in cc.ALL if cc.select(fam, fr)]


@pytest.mark.parametrize("fam, fr", PAIRS)
def test_frames_are_the_model(fam, fr):
    todo = cc.select(fam, fr)
    for c in todo:
        for level in c.levels: check(c, fr, level)
    print("%s %s: %d cases" % (fam, fr, len(todo)))


TEXT = [(c.name, fr, lvl) for c in cc.corpus() if c.fam == "text" for fr in c.framings for lvl in c.levels]


@pytest.mark.parametrize("name, fr, level", TEXT)
def test_text_frames_are_the_model(name, fr, level):
    check([c for c in cc.corpus() if c.name == name][0], fr, level)


def test_every_case_is_run():
    """Nothing is left out on the GPU that tests/test_hc_model_cpu.py covers: every case, framing and level is in one of the two tests."""
    ran = {(c.name, fr, lvl) for fam, fr in PAIRS for c in cc.select(fam, fr) for lvl in c.levels} | set(TEXT)
    assert ran == {(c.name, fr, lvl) for c in cc.corpus() for fr in c.framings for lvl in c.levels}
    assert {c.attempts for c in cc.corpus()} == {None, 1, 2, 3, 5}
