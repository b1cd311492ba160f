"""Every encoder's frames on the planted corpus of encoder_cases.py, held to the LZ4 writer rules (lz4_writer_rules.audit).

A round trip through the oracle cannot see a frame that breaks a writer's rule and still decodes, nor tell whether a branch of
passes S and E2 was reached at all.  So every frame here is audited, round-tripped (oracle and device decoder), bounded by
frame_bound, and - for the encoders that are functions of their input - its parse must be the planted one.

Encoders:  A   level 0, the shared finder (k_find_matches)            B   level 0, deterministic (solo_find_chunk)
           C3, C9, C12   the hash-chain levels                        D0, D9   compress_frames_async, a framing's cases in one batch
           E   the streaming ABI: one LZ4F_compressUpdate with the whole case, then LZ4F_compressEnd (k_layout_small)
Framings:  encoder_cases.FRAMINGS - 64 KiB independent, 64 KiB linked, 256 KiB linked with block checksums, 4 MiB independent with
           content checksum.  A case runs in the framings it is listed for.
Each (encoder, framing) is produced once and shared by the tests below; what is kept per frame is its verdicts, parse and digest.
"""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import oracle
import encoder_cases as ec
import lz4_writer_rules as wr
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_frame_conduit_amd.device import Engine, frame_windows
from lz4_index import Parsed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENCODERS = ("A", "B", "C3", "C9", "C12", "D0", "D9", "E")
LEVEL = {"A": 0, "B": 0, "C3": 3, "C9": 9, "C12": 12, "D0": 0, "D9": 9, "E": 0}
FUNCTIONS_OF_INPUT = ("B", "C3", "C9", "C12", "D0", "D9")
OUT_OF_REACH = ("off/D65536", "link/reach/D65536", "link/block3_repeats_block1")

# Forced cases an encoder does not parse as planted, each with the reason from its finder's code.  At most 1 in 16 per encoder, none
# from end, lit, carry or raw (test_exemptions_are_few_and_reasoned).
_SAME_STEP = ("the deterministic finder probes 64 positions per step and a lane does not see what the other lanes of its step insert "
              "(encode_solo.cuh, probe A): the one-byte run's source is the literal directly in front, in the plant's own step, and the "
              "plant is over before the next step")
EXEMPT = {
    "B": {"mlen/ovl/M19/D1": _SAME_STEP, "mlen/ovl/M20/D1": _SAME_STEP, "off/D1/M20": _SAME_STEP},
    "C3": {}, "C9": {}, "C12": {},
}
EXEMPT["D0"] = EXEMPT["B"]                                   # (the batch call runs the same finders)
EXEMPT["D9"] = EXEMPT["C9"]
A_EXEMPT = {}

_ENG, _DATA, _RUNS = {}, {}, {}


def engine(det: bool) -> Engine:
    if det not in _ENG:
        _ENG[det] = Engine(0)
        _ENG[det].set_deterministic(det)
    return _ENG[det]


def prefs(fr: str, level: int):
    f = ec.FRAMINGS[fr]
    return conduit.make_preferences(blockSizeID=f["bsid"], blockMode=0 if f["linked"] else 1, blockChecksum=int(f["bck"]),
                                    contentChecksum=int(f["cck"]), compressionLevel=level)


def inputs(fr: str):
    """[(case, data)] of a framing, built once."""
    if fr not in _DATA: _DATA[fr] = [(c, c.data) for c in ec.in_framing(fr)]
    return _DATA[fr]


def _single(eng, datas, p):
    """compress_async, input by input, through one source and one destination buffer."""
    cap_in = max(len(d) for d in datas)
    src = torch.zeros(cap_in + 16, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(eng.frame_bound(cap_in, p), dtype=torch.uint8, device=DEV)
    out = []
    for d in datas:
        n = len(d)
        if n: src[:n] = torch.frombuffer(bytearray(d), dtype=torch.uint8)
        eng.compress_async(src[:n], dst, p)
        r = eng.result()
        out.append(dst[:r.size].cpu().numpy().tobytes())
    return out


def _batch(eng, datas, p):
    lens = [len(d) for d in datas]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    do = frame_windows(lens, p, 0)
    src = torch.from_numpy(np.frombuffer(b"".join(datas) + bytes(16), dtype=np.uint8).copy()).to(DEV)
    dst = torch.zeros(do[-1], dtype=torch.uint8, device=DEV)
    res = eng.new_results(len(lens))
    eng.compress_frames_async(src, torch.from_numpy(so).to(DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), p, res)
    recs = eng.frame_results(res)
    assert all(r.status == 0 for r in recs), [(i, r.status) for i, r in enumerate(recs) if r.status]
    host = dst.cpu().numpy()
    return [host[do[i]:do[i] + recs[i].size].tobytes() for i in range(len(lens))]


def _stream(L, data: bytes, p) -> bytes:
    c = ctypes.c_void_p()
    assert L.LZ4F_createCompressionContext(ctypes.byref(c), 100) == 0
    hdr = ctypes.create_string_buffer(32)
    r = L.LZ4F_compressBegin(c, hdr, 32, ctypes.byref(p))
    assert not L.LZ4F_isError(r), L.LZ4F_getErrorName(r)
    out = [hdr.raw[:r]]
    if data:
        bound = L.LZ4F_compressBound(len(data), ctypes.byref(p))
        dst = ctypes.create_string_buffer(bound)
        r = L.LZ4F_compressUpdate(c, dst, bound, data, len(data), None)
        assert not L.LZ4F_isError(r), (L.LZ4F_getErrorName(r), L.lz4f_mi355x_last_error())
        out.append(dst.raw[:r])
    eb = L.LZ4F_compressBound(0, ctypes.byref(p))
    ed = ctypes.create_string_buffer(eb)
    r = L.LZ4F_compressEnd(c, ed, eb, None)
    assert not L.LZ4F_isError(r), L.LZ4F_getErrorName(r)
    out.append(ed.raw[:r])
    L.LZ4F_freeCompressionContext(c)
    return b"".join(out)


def _device_decode(eng, frame: bytes, n: int, back: torch.Tensor) -> bytes:
    src = torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).to(DEV)
    eng.decompress_frame_async(src, len(frame), back)
    r = eng.result()
    assert r.size == n, (r.size, n)
    return back[:n].cpu().numpy().tobytes()


def runs(enc: str, fr: str) -> dict:
    """case name -> what its frame showed: violations, round-trip verdict, size against the bound, merged parse, shapes, digest."""
    if (enc, fr) in _RUNS: return _RUNS[enc, fr]
    todo = inputs(fr)
    if enc == "E": todo = [(c, d) for c, d in todo if len(d) <= 3 * ec.BS[fr]]
    datas = [d for _, d in todo]
    p = prefs(fr, LEVEL[enc])
    eng = engine(enc != "A")
    if enc[0] == "D": frames = _batch(eng, datas, p)
    elif enc == "E": frames = [_stream(_ffi.lib(), d, p) for d in datas]
    else: frames = _single(eng, datas, p)
    back = torch.zeros(max(len(d) for d in datas) + 64, dtype=torch.uint8, device=DEV)
    out = {}
    for (c, data), frame in zip(todo, frames):
        rec = dict(size=len(frame), bound=eng.frame_bound(len(data), p), n=len(data), sha=hashlib.sha256(frame).hexdigest(), merged=None, shapes=set())
        try:
            P = Parsed(frame)
        except Exception:
            P = None
        rec["audit"] = wr.audit(frame, data, ec.FRAMINGS[fr], P)
        if P is not None:
            rec["merged"] = wr.matches(frame, P)
            rec["shapes"] = ec.shapes(P, rec["merged"])
        try:
            got, used = oracle.decompress_frame(frame, cap=len(data) + 64)
            rec["round_trip"] = "" if (got == data and used == len(frame)) else "the oracle gives %d bytes back, uses %d of %d" % (len(got), used, len(frame))
        except oracle.OracleError as e:
            rec["round_trip"] = "the oracle refuses it: %s" % e
        if data and not rec["round_trip"] and _device_decode(eng, frame, len(data), back) != data: rec["round_trip"] = "the device decoder gives other bytes back"
        out[c.name] = rec
    _RUNS[enc, fr] = out
    return out


def forced(fr: str):
    return [c for c, _ in inputs(fr) if c.forced]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fr", list(ec.FRAMINGS))
@pytest.mark.parametrize("enc", ENCODERS)
def test_frames_keep_the_writer_rules_and_round_trip(enc, fr):
    """Every frame: no violation of a writer rule, the oracle and decompress_frame_async give the input back, the frame is within
    frame_bound; a repeat that is 65536 back is not used (the frame is no smaller than the input, and no offset is 0 - the audit)."""
    R = runs(enc, fr)
    assert len(R) > 50
    bad = {n: r["audit"] for n, r in R.items() if r["audit"]}
    assert not bad, (len(bad), dict(list(bad.items())[:5]))
    bad = {n: r["round_trip"] for n, r in R.items() if r["round_trip"]}
    assert not bad, (len(bad), dict(list(bad.items())[:5]))
    assert all(r["size"] <= r["bound"] for r in R.values()), [n for n, r in R.items() if r["size"] > r["bound"]]
    for n in OUT_OF_REACH:
        if n in R: assert R[n]["size"] >= R[n]["n"] and "stored" in R[n]["shapes"], (n, R[n]["size"], R[n]["n"])


@pytest.mark.parametrize("fr", list(ec.FRAMINGS))
@pytest.mark.parametrize("batch, single", [("D0", "B"), ("D9", "C9")])
def test_batch_frames_are_the_single_calls(batch, single, fr):
    """Byte for byte.  This is also where pass E2's two instantiations meet: a call of up to 512 chunks - every single call of this
    file - launches k_emit_gather<W, true> (`split`: a workgroup's waves share one chunk, engine.hip's e2_split), the batch call
    runs emit_chunk<false>, a wave per chunk (encode_batch.cuh): every case goes through both, and their bytes must agree."""
    D, S = runs(batch, fr), runs(single, fr)
    assert D.keys() == S.keys()
    assert [n for n in D if D[n]["sha"] != S[n]["sha"]] == []


@pytest.mark.parametrize("fr", list(ec.FRAMINGS))
@pytest.mark.parametrize("enc", FUNCTIONS_OF_INPUT)
def test_parse_is_the_planted_one(enc, fr):
    """The deterministic, hash-chain and batch encoders are functions of the input: on every forced case the merged parse is the
    planted (position, M, D, L) list - but for the cases EXEMPT names, with their reasons.  The cases of 4 MiB and more (their
    background is not searched for chance repeats) must hold every plant as (position, M, D) and be within 256 bytes of the planted
    parse's frame: a chance 4-byte repeat within reach moves the size by a byte or two, and some 64 are to be expected in 4 MiB."""
    R = runs(enc, fr)
    missed = {}
    for c in forced(fr):
        if c.name in EXEMPT[enc]: continue
        got = [tuple(r) for r in R[c.name]["merged"].tolist()]
        want = c.expected(ec.BS[fr])
        if got != want:
            k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            missed[c.name] = (len(got), len(want), got[k:k + 2], want[k:k + 2])
    for c, _ in inputs(fr):                                   # 4 MiB and more: no whole parse is claimed, but every plant is written, and little else
        if c.forced or not c.build()[1]: continue
        got = {tuple(r[:3]) for r in R[c.name]["merged"].tolist()}
        lost = [w for w in c.expected(ec.BS[fr]) if w[:3] not in got]
        want = ec.planted_frame_size(c, fr)
        print("%s %s %s: %d bytes, planted %d" % (enc, fr, c.name, R[c.name]["size"], want))
        if lost or abs(R[c.name]["size"] - want) > 256: missed[c.name] = (lost, R[c.name]["size"], want)
    print("%s %s: %d forced cases, %d missed" % (enc, fr, len(forced(fr)), len(missed)))
    for n, v in missed.items(): print("   ", n, v)
    assert not missed, (len(missed), dict(list(missed.items())[:4]))


@pytest.mark.parametrize("fr", list(ec.FRAMINGS))
def test_shared_finder_finds_the_long_plants(fr):
    """Encoder A's short finds are a matter of timing; a plant of 4096 bytes and more it must find: matches at the plant's distance
    (for a plant that overlaps its source, D < M: at a multiple of it) cover at least half of it."""
    R = runs("A", fr)
    missed = {}
    for c in forced(fr):
        if c.name in A_EXEMPT: continue
        m = R[c.name]["merged"]
        for pos, M, D, _ in c.expected(ec.BS[fr]):
            if M < ec.A_HELD: continue
            same = m[m[:, 2] == D] if D >= M else m[m[:, 2] % D == 0]       # (a periodic plant repeats at every multiple of D as well)
            cover = int(np.clip(np.minimum(same[:, 0] + same[:, 1], pos + M) - np.maximum(same[:, 0], pos), 0, None).sum())
            if cover * 2 < M: missed[c.name] = (pos, M, D, cover)
    print("A %s: missed" % fr, missed)
    assert not missed, missed


def test_exemptions_are_few_and_reasoned():
    names = {c.name: c for c in ec.corpus()}
    n_forced = sum(c.forced for c in ec.corpus())
    for enc, ex in list(EXEMPT.items()) + [("A", A_EXEMPT)]:
        assert len(ex) * 16 <= n_forced, (enc, len(ex), n_forced)
        for n, why in ex.items():
            assert n in names and names[n].forced and len(why) > 40, (enc, n)
            assert names[n].fam not in ("end", "lit", "carry", "raw"), (enc, n)


def test_shapes_written():
    """Counted from the parsed frames, per encoder: every literal-run, match-length and offset threshold, a match starting exactly at
    blen - 12 and one ending at blen - 5, a carry across each length-byte threshold, a stored block, the lengths of pass E2's scalar
    branch and both of its paths.  B, C and D must show each; A's list is printed."""
    seen = {enc: set().union(*(r["shapes"] for fr in ec.FRAMINGS for r in runs(enc, fr).values())) for enc in ENCODERS}
    print("A wrote:", [s for s in ec.SHAPES if s in seen["A"]])
    print("A did not write:", [s for s in ec.SHAPES if s not in seen["A"]])
    print("E did not write:", [s for s in ec.SHAPES if s not in seen["E"]])
    lacking = {enc: [s for s in ec.SHAPES if s not in seen[enc]] for enc in FUNCTIONS_OF_INPUT}
    assert not any(lacking.values()), lacking
