"""The measure call's yardstick and host side, without a device.

tests/measure_model.py is what the GPU tests hold lz4f_mi355x_dev_measureFrames to, so it is held to the oracle first: over the
block grammar's corpus, the frame grammar's, the golden files and oracle-made frames of every framing, the model accepts what
the oracle accepts (with the oracle's size), rejects nothing the oracle accepts, and what it accepts but the oracle rejects is
rejected for a match offset or a checksum - the three things measure does not look at - and for nothing else.
Then Engine.measure_frames_async's argument checks."""
import ctypes

import pytest
import torch

import measure_model as mm
import oracle
from lz4_frame_conduit_amd import _ffi
from lz4_frame_conduit_amd._ffi import Result
from lz4_frame_conduit_amd.device import Engine

REC = ctypes.sizeof(Result)
CHECKSUM_ERRORS = ("ERROR_blockChecksum_invalid", "ERROR_contentChecksum_invalid")


@pytest.fixture(scope="module")
def verdicts():
    """[(name, frame, model, (oracle error, oracle output, oracle consumed))]"""
    return [(n, f, mm.model_of(f), mm.oracle_verdict(f)) for n, f in mm.frames()]


def test_corpus_has_every_kind(verdicts):
    names = [n for n, _, _, _ in verdicts]
    for prefix in ("grammar/end/", "grammar/off/", "grammar/link/", "grammar/blk/", "edges/trunc/", "edges/skip/", "golden/", "made/b7/i0/k3", "made/empty/",
                   "made/skippable_first"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert len(names) > 800


def test_model_accepts_what_the_oracle_accepts(verdicts):
    n_ok = 0
    for name, f, m, (err, out, used) in verdicts:
        if err is None:
            n_ok += 1
            assert m.status == 0, (name, m)
            assert (m.size, m.consumed) == (len(out), used), (name, m, len(out), used)
            bs = 1 << (8 + 2 * ((f[5] >> 4) & 7)) if m.n_blocks else 0
            assert m.size <= m.W <= m.n_blocks * bs, (name, m)
    assert n_ok > len(verdicts) // 3


def test_oracle_rejects_what_the_model_rejects(verdicts):
    n_bad = 0
    for name, f, m, (err, out, used) in verdicts:
        if m.status != 0:
            n_bad += 1
            assert err is not None, (name, m)
            assert m.W == 0
    assert n_bad > 100


def test_model_only_misses_offsets_and_checksums(verdicts):
    """A frame the model accepts and the oracle rejects: the oracle names a checksum; or, with every match offset made valid
    (and the block checksums made right for the new bytes), the oracle accepts it with the model's size or is down to the
    content checksum of the bytes that have changed - or, where a match sits where no offset is valid, decodes every block given
    one byte of history.  Below a fifth of what the oracle rejects: the model is no rubber stamp."""
    rejected = [v for v in verdicts if v[3][0] is not None]
    missed = [v for v in rejected if v[2].status == 0]
    by = {"checksum": 0, "offset": 0}
    for name, f, m, (err, _, _) in missed:
        if err in CHECKSUM_ERRORS:
            by["checksum"] += 1
            continue
        assert err in ("ERROR_GENERIC", "ERROR_decompressionFailed"), (name, err)
        g, payloads, hopeless = mm.with_valid_offsets(f)
        assert g != f and len(g) == len(f), name
        assert mm.model_of(g)[:6] == m[:6], name                                   # (offsets and checksums: nothing the model looks at)
        if hopeless:
            # a match at a block's very start with nothing in front of it: no offset is valid there.  With one byte of history
            # every block decodes, to what the model says
            bs = 1 << (8 + 2 * ((f[5] >> 4) & 7))
            for payload, got in payloads:
                assert len(oracle.decompress_block(payload, bs, history=b"h")) == got, name
        else:
            err2, out2, used2 = mm.oracle_verdict(g)
            assert err2 is None or err2 == "ERROR_contentChecksum_invalid", (name, err, err2)
            if err2 is None:
                assert (len(out2), used2) == (m.size, m.consumed), name
        by["offset"] += 1
        assert hopeless or name.startswith(("grammar/off/", "grammar/link/")), name     # (and by name: the families that plant a wrong offset)
        print("   ", name, err, "no valid offset" if hopeless else "")
    print("oracle rejects %d, of which the model accepts %d: %s" % (len(rejected), len(missed), by))
    assert by["checksum"] and by["offset"]
    assert len(missed) * 5 < len(rejected), (len(missed), len(rejected))


def test_the_decoders_bound_on_blocks_per_span():
    """Not the format's rule but the batch decoder's, window or no window: block number span / 5 + 2 is one too many.  Only empty
    stored blocks are small enough to get there; the oracle accepts such a frame, the model must say what the decoder will."""
    for linked in (False, True):
        for n, status in ((3, 0), (21, 0), (22, mm.DSTSMALL), (60, mm.DSTSMALL)):
            f = mm.empty_stored_frame(n, linked=linked)
            assert len(f) == 11 + 4 * n and mm.oracle_verdict(f) == (None, b"", len(f))
            m = mm.measure(f)
            assert m.status == status == (mm.DSTSMALL if n - 1 >= len(f) // 5 + 2 else 0), (n, m)
            assert tuple(m) == ((0, 0, len(f), n, mm.NONE, f[4], (n - 1) * 65536 + 1) if status == 0 else (mm.DSTSMALL, 0, 0, 0, mm.NONE, f[4], 0))


def test_window_rule():
    bs = 1 << 16
    # every block but the last full: the size
    assert mm.window([bs, bs, 77], bs, False) == 2 * bs + 77 and mm.window([bs, bs, 77], bs, True) == 2 * bs + 77
    assert mm.window([bs], bs, False) == bs and mm.window([], bs, True) == 0
    # short inner blocks: every block's place inside the window; an independent block decodes at its place
    assert mm.window([5000] * 7, bs, False) == 6 * bs + 5000 and mm.window([5000] * 7, bs, True) == 6 * bs + 1
    assert mm.window([bs, 0, 9000], bs, True) == 2 * bs + 1 and mm.window([bs, bs - 1, 9000], bs, True) == 2 * bs + 8999
    # a last block of nothing still needs its place
    assert mm.window([bs, 0], bs, False) == bs + 1 and mm.window([0], bs, True) == 1
    for gots in ([5000] * 7, [bs, 0, 9000], [bs, bs, 77], [3, bs, 1]):
        for linked in (False, True):
            w = mm.window(gots, bs, linked)
            assert mm.decoder_accepts(gots, bs, linked, w) and not mm.decoder_accepts(gots, bs, linked, w - 1) and w <= len(gots) * bs


# ---- Engine.measure_frames_async: the argument checks ----
def _engine():
    e = Engine.__new__(Engine)              # (no device: the checks come before anything touches one)
    e.h = None
    return e


def _args(n=3, **kw):
    a = dict(src=torch.zeros(100, dtype=torch.uint8), src_off=torch.zeros(n + 1, dtype=torch.int64), results=torch.zeros(n * REC, dtype=torch.uint8),
             dst_off=torch.zeros(n + 1, dtype=torch.int64))
    a.update(kw)
    return a


def test_symbol_is_declared():
    assert "lz4f_mi355x_dev_measureFrames" in _ffi.DECLARED_SYMBOLS


def test_null_engine_is_a_call_error():
    L = _ffi.lib()
    off = (ctypes.c_uint64 * 2)(0, 0)
    assert L.LZ4F_isError(L.lz4f_mi355x_dev_measureFrames(None, 1, None, 0, off, None, None))
    assert L.LZ4F_isError(L.lz4f_mi355x_dev_measureFrames(None, 0, None, 0, None, None, None))


@pytest.mark.parametrize("bad, msg", [
    (dict(src=torch.zeros(100, dtype=torch.int8)), "src must be torch.uint8"),
    (dict(src_off=torch.zeros(4, dtype=torch.int32)), "src_off must be torch.int64"),
    (dict(dst_off=torch.zeros(4, dtype=torch.uint8)), "dst_off must be torch.int64"),
    (dict(results=torch.zeros(96, dtype=torch.int32)), "results must be torch.uint8"),
    (dict(src=torch.zeros(10, 10, dtype=torch.uint8)), "contiguous 1-d"),
    (dict(dst_off=torch.zeros(8, dtype=torch.int64)[::2]), "contiguous 1-d"),
    (dict(src_off=torch.zeros(0, dtype=torch.int64), dst_off=None), "n\\+1 offsets"),
    (dict(dst_off=torch.zeros(3, dtype=torch.int64)), "n\\+1 offsets"),
    (dict(results=torch.zeros(3 * 32 - 1, dtype=torch.uint8)), "results must hold 96 bytes for 3 frames"),
    (dict(src=[0] * 100), "src must be a tensor"),
    (dict(dst_off=[0] * 4), "dst_off must be a tensor"),
])
def test_wrapper_rejects(bad, msg):
    with pytest.raises(ValueError, match=msg):
        _engine().measure_frames_async(**_args(**bad))


def test_wrapper_wants_device_memory():
    with pytest.raises(ValueError, match="device memory"):
        _engine().measure_frames_async(**_args())
    with pytest.raises(ValueError, match="device memory"):
        _engine().measure_frames_async(**_args(dst_off=None))
    with pytest.raises(ValueError, match="device memory"):
        _engine().measure_frames_async(**_args(n=0, results=torch.zeros(0, dtype=torch.uint8)))
