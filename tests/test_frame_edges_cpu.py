"""The host-side frame parsers on the frame-edge corpus (tests/frame_edges.py), against the oracle's header parse and walk.

LZ4F_headerSize, LZ4F_getFrameInfo and lz4f_mi355x_blockListSize read a frame without decoding it, so each is held to the part of
the oracle's verdict it can see.  Where an entry point answers differently from the oracle's one-shot decoder for a whole CLASS
of cases, the class is pinned by rule below, with the oracle's answer beside it.  No GPU."""
import ctypes
import itertools

import pytest

import frame_edges as fe
import oracle
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_frame_conduit_amd._ffi import FrameInfo

INCOMPLETE = "ERROR_frameHeader_incomplete"
# what only a decode can find: a parser that walks the size words does not see these
DECODE_ERRORS = {"ERROR_blockChecksum_invalid", "ERROR_contentChecksum_invalid", "ERROR_frameSize_wrong", "ERROR_dstMaxSize_tooSmall",
                 "ERROR_GENERIC", "ERROR_decompressionFailed"}


@pytest.fixture(scope="module")
def L():
    _ffi.build()
    return _ffi.lib()


def err_of(L, r):
    return L.LZ4F_getErrorName(r).decode() if L.LZ4F_isError(r) else None


def info_tuple(i):
    return (i.blockSizeID, i.blockMode, i.contentChecksumFlag, i.frameType, i.contentSize, i.dictID, i.blockChecksumFlag)


def trailer_size(frame_len, n_blocks):
    """lz4f_mi355x.h, "the trailer": magic, size, pad to 16, one u64 per block (an even number of them), a 32-byte footer."""
    if n_blocks == 0:
        return 0
    list_at = (frame_len + 8 + 15) & ~15
    return list_at + ((n_blocks + 1) & ~1) * 8 + 32 - frame_len


def test_header_size(L):
    for name, f, w in fe.corpus():
        v = fe.verdict(f, w)
        got = L.LZ4F_headerSize(f, len(f))
        if len(f) < 5:
            # liblz4: LZ4F_headerSize needs 5 bytes (magic and FLG) whatever they are.  Oracle: frameHeader_incomplete too
            assert err_of(L, got) == INCOMPLETE == v.error, name
        elif fe.is_skippable(f):
            # class "skippable": a skippable frame's header is its 8 bytes, cut or not.  Oracle: consumes 8 + payload, or
            # frameHeader_incomplete when cut
            assert got == 8, name
        elif v.error == "ERROR_frameType_unknown":
            assert err_of(L, got) == v.error, name
        else:
            # class "length only": the length comes from FLG's two option bits; nothing else is judged (liblz4's LZ4F_headerSize).
            # Oracle: judges the whole descriptor - where it accepts it, its own header for that frame info has this length
            assert got == fe.hsize(f), name
            if v.header_ok:
                i = v.info
                p = oracle.mkprefs(bsid=i.blockSizeID, indep=i.blockMode, cck=i.contentChecksumFlag, bck=i.blockChecksumFlag, csize=i.contentSize, dictid=i.dictID)
                assert got == len(oracle.header_bytes(p)), name


def test_get_frame_info(L):
    for name, f, w in fe.corpus():
        v = fe.verdict(f, w)
        d = ctypes.c_void_p()
        assert L.LZ4F_createDecompressionContext(ctypes.byref(d), 100) == 0
        try:
            info, n = FrameInfo(), ctypes.c_size_t(len(f))
            r = L.LZ4F_getFrameInfo(d, ctypes.byref(info), f, ctypes.byref(n))
        finally:
            L.LZ4F_freeDecompressionContext(d)
        got = err_of(L, r)
        if fe.is_skippable(f) and len(f) >= 8:
            # class "skippable": the frame type is known from the magic and the size word; the payload is not looked at.
            # Oracle: frameHeader_incomplete for a cut payload, else frame type 1 as here
            assert got is None and info.frameType == 1, name
            if v.error is None:
                assert v.info.frameType == 1, name
        elif v.header_ok:
            # whatever is wrong behind the header is not this call's business
            assert got is None and n.value == fe.hsize(f), (name, got)
            assert info_tuple(info) == info_tuple(v.info), name
        else:
            assert got == v.error and n.value == 0, (name, got, v.error)


def test_block_list_size(L):
    for name, f, w in fe.corpus():
        v = fe.verdict(f, max(w, 1 << 17))                          # (a window that holds the content: the walk has none)
        got = L.lz4f_mi355x_blockListSize(f, len(f))
        if fe.is_skippable(f) and len(f) >= 7:
            # class "skippable": a skippable frame has no blocks to list: frameType_unknown.  Oracle: accepts it (no output), or
            # frameHeader_incomplete when cut
            assert err_of(L, got) == "ERROR_frameType_unknown", name
        elif v.error is None or v.error in DECODE_ERRORS:
            # class "walk only": the list is made from the size words; payloads, checksums and the content size are not looked at.
            # Oracle: names the decode error
            assert err_of(L, got) is None, (name, err_of(L, got))
            assert got == trailer_size(len(f), len(fe.blocks_of(f))), name
        else:
            assert err_of(L, got) == v.error, (name, err_of(L, got), v.error)


PREFS = list(itertools.product((0, 4, 5, 6, 7), (0, 1), (0, 1), (0, 1), (0, 1, 70000, (1 << 40) + 5), (0, 1, fe.DICT_ID)))


def test_compress_begin_header(L):
    for bsid, indep, bck, cck, csize, dictid in PREFS:
        kw = dict(bsid=bsid, indep=indep, bck=bck, cck=cck, csize=csize, dictid=dictid)
        want = oracle.header_bytes(oracle.mkprefs(**kw))
        p = conduit.make_preferences(blockSizeID=bsid, blockMode=indep, contentChecksum=cck, blockChecksum=bck, contentSize=csize, dictID=dictid)
        c = ctypes.c_void_p()
        assert L.LZ4F_createCompressionContext(ctypes.byref(c), 100) == 0
        try:
            buf = ctypes.create_string_buffer(32)
            r = L.LZ4F_compressBegin(c, buf, 32, ctypes.byref(p))
        finally:
            L.LZ4F_freeCompressionContext(c)
        assert not L.LZ4F_isError(r) and buf.raw[:r] == want, kw
        # ... and parses back
        assert L.LZ4F_headerSize(want, len(want)) == len(want), kw
        d = ctypes.c_void_p()
        assert L.LZ4F_createDecompressionContext(ctypes.byref(d), 100) == 0
        try:
            info, n = FrameInfo(), ctypes.c_size_t(len(want))
            r = L.LZ4F_getFrameInfo(d, ctypes.byref(info), want, ctypes.byref(n))
        finally:
            L.LZ4F_freeDecompressionContext(d)
        assert not L.LZ4F_isError(r) and n.value == len(want), kw
        assert info_tuple(info) == (bsid or 4, indep, cck, 0, csize, dictid, bck), kw
