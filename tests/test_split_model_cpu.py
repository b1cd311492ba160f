"""tests/split_model.py - what lz4f_mi355x_dev_splitFrames computes - held to the oracle, and its shared cases held to what their
builders planted, so that tests/test_gpu_split_frames.py cannot inherit a wrong expectation.  And the call's C ABI as far as it goes
without a device: declared, exported, bound, and refusing a null engine."""
import ctypes
import os
import re

import pytest

import oracle
import split_model as sm
from lz4_frame_conduit_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL, HOST_SYMBOL = "lz4f_mi355x_dev_splitFrames", "lz4f_mi355x_splitFrames"


@pytest.fixture(scope="module")
def cases():
    return sm.all_cases()


def test_listed_spans_decode_with_the_oracle_and_end_where_the_model_says():
    made = sm.oracle_frames()
    stream = b"".join([sm.skippable(b"in front", 1)] + [f + (sm.skippable(b"behind", k) if k % 3 == 0 else b"") for k, (_, f, _) in enumerate(made)])
    w = sm.walk(stream)
    assert w.status == 0 and w.pos == len(stream) and len(w.starts) == len(made) and w.skipped and w.bytes == sum(len(f) for _, f, _ in made)
    ends = w.starts[1:] + [w.pos]
    for (prefs, f, x), a, b in zip(made, w.starts, ends):
        out, used = oracle.decompress_frame(stream[a:b], cap=len(x) + 16)
        assert out == x, prefs
        assert sm.step(stream, a) == ("frame", used), prefs                   # the model's frame ends where the oracle stopped reading
        assert stream[a:a + used] == f


def test_model_stops_where_the_oracle_refuses():
    """The statuses of a stop are the oracle's errors for the same bytes (where the oracle's decode needs no more than the walk reads)"""
    names = {sm.ST_INCOMPLETE: ("ERROR_frameHeader_incomplete", "ERROR_srcSize_tooSmall", "incomplete"), sm.ST_FRAMETYPE: ("ERROR_frameType_unknown",),
             sm.ST_RESERVED: ("ERROR_reservedFlag_set",), sm.ST_VERSION: ("ERROR_headerVersion_wrong",), sm.ST_MAXBLOCK: ("ERROR_maxBlockSize_invalid",),
             sm.ST_HEADERCK: ("ERROR_headerChecksum_invalid",)}
    seen = set()
    for c in sm.stop_streams():
        w = sm.walk(c.stream)
        if c.name in ("stop/skippable_cut",) or w.status == sm.ST_INCOMPLETE:
            continue                                                           # (a cut: the oracle's streaming decode asks for more input, its own way)
        with pytest.raises(oracle.OracleError) as e:
            oracle.decompress_frame(c.stream[w.pos:], cap=1 << 16)
        assert any(n in str(e.value) for n in names[w.status]), (c.name, str(e.value), w.status)
        seen.add(w.status)
    assert seen == {sm.ST_FRAMETYPE, sm.ST_RESERVED, sm.ST_VERSION, sm.ST_MAXBLOCK, sm.ST_HEADERCK}


def test_every_case_is_what_its_builder_planted(cases):
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert sm.walk(c.stream) == c.planted, c.name
        n = len(c.planted.starts)
        off, rec = sm.split(c.stream, n if c.max_frames is None else c.max_frames)
        assert rec.n_blocks == n and rec.consumed == c.planted.pos and rec.size == c.planted.bytes, c.name
    by = {c.name: c for c in cases}
    assert by["stop/word_above_block_size/3"].planted.status == sm.ST_MAXBLOCK and len(by["stop/word_above_block_size/3"].planted.starts) == 3
    assert by["stop/legacy"].planted.status == sm.ST_FRAMETYPE and by["stop/2_bytes_behind"].planted.status == sm.ST_INCOMPLETE
    assert by["stop/at_once"].planted == sm.Walk([], 0, sm.ST_FRAMETYPE, 0, False)
    assert len(by["depth/66000"].planted.starts) == 66000 and len(by["depth/66000"].stream) == 726000
    assert [len(c.planted.starts) for c in cases if c.name.startswith("false/")] == [4, 3, 3, 3]
    assert [sm.nodes(c.stream) - len(c.planted.starts) for c in cases if c.name.startswith("false/")] == [4, 1, 7, 1]      # the false nodes: 4 inner frames; 1; 3 + 1 + 3 levels; the header that stands alone


def test_output_rules():
    c = next(c for c in sm.max_frames_cases())
    w, n = c.planted, 6
    assert len(w.starts) == n and w.starts[0] == 48
    off, rec = sm.outputs(w, n)
    assert off == w.starts + [w.pos] and rec == sm.Rec(0, w.bytes, w.pos, n, sm.NONE, sm.FLAG_SKIPPABLE)
    off, rec = sm.outputs(w, n - 1)
    assert off == w.starts[:n - 1] + [w.starts[n - 1]] and rec.status == sm.ST_DSTSMALL and rec.n_blocks == n and rec.first_bad_block == sm.NONE
    off, rec = sm.outputs(w, 1)
    assert off == [w.starts[0], w.starts[1]] and rec.status == sm.ST_DSTSMALL
    off, rec = sm.outputs(w, 4 * n)
    assert off == w.starts + [w.pos] * (3 * n + 1) and rec.status == 0
    bad = sm.five(3).planted()                                                  # a grammar error wins over "more frames than asked for"
    off, rec = sm.outputs(bad, 2)
    assert rec == sm.Rec(sm.ST_MAXBLOCK, bad.bytes, bad.pos, 3, 3, 0) and off == bad.starts[:2] + [bad.starts[2]]
    assert sm.split(b"", 2) == ([0, 0, 0], sm.Rec(0, 0, 0, 0, sm.NONE, 0))


def test_truncations_and_overflow_are_what_they_claim():
    stream, a = sm.truncation_stream()
    for cut in range(a + 1, len(stream)):
        assert sm.walk(stream[:cut]) == sm.Walk([0], a, sm.ST_INCOMPLETE, a, False), cut
    assert sm.walk(stream[:a]) == sm.Walk([0], a, 0, a, False) and len(sm.walk(stream).starts) == 2
    c = sm.overflow_case()
    assert c.serial and sm.nodes(c.stream) > sm.node_cap(c.max_frames, len(c.stream)) + 9000
    for c in sm.all_cases():
        if not c.serial and len(c.stream) < 200000:
            mf = len(c.planted.starts) if c.max_frames is None else c.max_frames
            assert sm.nodes(c.stream) <= sm.node_cap(mf, len(c.stream)), c.name      # every other case fits its node list


# ---- the C ABI ----
@pytest.fixture(scope="module")
def L():
    _ffi.build()
    return _ffi.lib()


def test_header_declares_and_library_exports(L):
    hdr = open(os.path.join(ROOT, "include", "lz4f_mi355x.h")).read()
    declared = set(re.findall(r"^LZ4F_MI355X_API[^;(]*?\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", hdr, flags=re.M))
    assert SYMBOL in declared and HOST_SYMBOL in declared
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), SYMBOL) and hasattr(ctypes.CDLL(_ffi.LIB_PATH), HOST_SYMBOL)
    assert int(re.search(r"#define\s+LZ4F_MI355X_SPLIT_SHARE\s+(\d+)u", hdr).group(1)) == sm.SPLIT_SHARE


def test_ffi_gives_argument_types_and_null_engine_is_refused(L):
    assert SYMBOL in _ffi.DECLARED_SYMBOLS
    f = getattr(L, SYMBOL)
    assert len(f.argtypes) == 6 and f.restype is ctypes.c_size_t
    for r in (f(None, None, 0, 0, None, None), f(None, None, 10, 3, None, None)):
        assert L.LZ4F_isError(r) and L.LZ4F_getErrorName(r) == b"ERROR_GENERIC"


def test_host_walk_is_the_model(L, cases):
    """lz4f_mi355x_splitFrames, the same walk over host memory by the library's own grammar: every case, offsets and record"""
    f = getattr(L, HOST_SYMBOL)
    assert HOST_SYMBOL in _ffi.DECLARED_SYMBOLS and len(f.argtypes) == 5
    stream, a = sm.truncation_stream()
    todo = [(c.stream, m) for c in cases for m in ({1, max(len(c.planted.starts), 1), len(c.planted.starts) + 3} | ({c.max_frames} if c.max_frames else set()))]
    todo += [(stream[:cut], 2) for cut in range(a, len(stream) + 1)] + [(b"", 2)]
    for S, m in todo:
        off = (ctypes.c_uint64 * (m + 3))(*([7] * (m + 3)))
        rec = _ffi.Result()
        buf = ctypes.create_string_buffer(S, len(S) + 1)
        assert f(buf, len(S), m, off, ctypes.byref(rec)) == 0
        want_off, want_rec = sm.split(S, m)
        assert list(off) == want_off + [7, 7]
        assert sm.Rec(rec.status, rec.size, rec.consumed, rec.n_blocks, rec.first_bad_block, rec.flags) == want_rec
    assert f(None, 0, 0, None, None) == 0 and L.LZ4F_isError(f(None, 5, 1, None, None))
