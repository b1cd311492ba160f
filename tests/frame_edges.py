"""The LZ4 frame grammar's edges: one small base frame, one planted defect per case.

corpus() -> [(name, frame bytes, window)].  Everything is cut from, or patched into, one base frame made by the oracle:
block size ID 4, independent blocks, block checksums, content checksum, content size and dictID, two blocks of 300 bytes.
A defect in the descriptor comes with the header checksum recomputed, so that it is the only defect.  verdict() is what the
oracle (oracle/orc_lz4frame.c) says about a case; nothing here touches the library under test or a GPU.

The frame layout is restated here on purpose (no helper of the library, none of the other tests' walks)."""
import ctypes
import functools

import oracle

MAGIC, SKIP0 = 0x184D2204, 0x184D2A50
DICT_ID = 0x0D1C7E57
BS = 1 << 16                       # block size ID 4


def le32(v: int) -> bytes:
    return (v & 0xFFFFFFFF).to_bytes(4, "little")


def base_data() -> bytes:
    # two blocks of 300 bytes, each a 50-byte phrase and echoes of it: literals, short and long matches, a few dozen payload bytes
    out, x = bytearray(), 12345
    for _ in range(2):
        phrase = bytearray()
        for _ in range(50):
            x = (x * 1103515245 + 12345) & 0x7FFFFFFF
            phrase.append(97 + (x >> 16) % 26)
        out += phrase + phrase[10:40] + phrase[::-1][:20] + phrase * 4
    return bytes(out)


def prefs(csize=0, dictid=0, cck=0, bck=1, bsid=4, indep=1, autoflush=0):
    return oracle.mkprefs(bsid=bsid, indep=indep, bck=bck, cck=cck, csize=csize, dictid=dictid, autoflush=autoflush)


@functools.lru_cache(maxsize=None)
def base_frame() -> bytes:
    d = base_data()
    f = oracle.conduit_compress(d, prefs(csize=len(d), dictid=DICT_ID, cck=1, autoflush=1), slice_=300)
    assert hsize(f) == 19 and len(blocks_of(f)) == 2
    return f


def hsize(f: bytes) -> int:
    return 7 + (8 if f[4] & 8 else 0) + (4 if f[4] & 1 else 0)


def blocks_of(f: bytes):
    """[(position of the size word, size word)] of a well-formed frame."""
    pos, out, crc = hsize(f), [], 4 if f[4] & 0x10 else 0
    while True:
        w = int.from_bytes(f[pos:pos + 4], "little")
        if w == 0:
            return out
        out.append((pos, w))
        pos += 4 + (w & 0x7FFFFFFF) + crc


def end_of_blocks(f: bytes) -> int:
    p, w = blocks_of(f)[-1]
    return p + 4 + (w & 0x7FFFFFFF) + (4 if f[4] & 0x10 else 0)


def reseal(f) -> bytes:
    """The frame with its header checksum made right for the descriptor it now has."""
    f = bytearray(f)
    h = hsize(f)
    f[h - 1] = (oracle.xxh32(bytes(f[4:h - 1])) >> 8) & 0xFF
    return bytes(f)


def patched(f: bytes, at: int, value: bytes, seal: bool = False) -> bytes:
    g = bytearray(f)
    g[at:at + len(value)] = value
    return reseal(g) if seal else bytes(g)


def is_skippable(f: bytes) -> bool:
    return len(f) >= 4 and int.from_bytes(f[:4], "little") & 0xFFFFFFF0 == SKIP0


def skippable(k: int, payload: bytes) -> bytes:
    return le32(SKIP0 + k) + le32(len(payload)) + payload


def stored_full_block_frame() -> bytes:
    """One stored block of exactly maxBlockSize, every option on."""
    d = (base_data() * (BS // 600 + 1))[:BS]
    head = oracle.header_bytes(prefs(csize=BS, dictid=DICT_ID, cck=1))
    return head + le32(0x80000000 | BS) + d + le32(oracle.xxh32(d)) + le32(0) + le32(oracle.xxh32(d))


COMBOS = [(c, d, k) for c in (0, 1) for d in (0, 1) for k in (0, 1)]      # content size x dictID x content checksum


def combo_prefs(c, d, k, n):
    return prefs(csize=n if c else 0, dictid=DICT_ID if d else 0, cck=k)


@functools.lru_cache(maxsize=None)
def corpus():
    base, data = base_frame(), base_data()
    n, W = len(base), len(data)
    out = []
    # The window, unless a case is about the window: every block's full room.  The device calls decode block i at its provisional
    # place, i * maxBlockSize, so a frame of short blocks needs that much to be judged by its defect and not by its window.
    add = lambda name, frame, window=2 * BS: out.append((name, bytes(frame), window))
    for k in range(n):
        add("trunc/%03d" % k, base[:k])
    # FLG
    add("flg/reserved", patched(base, 4, bytes([base[4] | 2]), seal=True))
    for v in (0, 2, 3):
        add("flg/version%d" % v, patched(base, 4, bytes([(base[4] & 0x3F) | (v << 6)]), seal=True))
    for c, d, k in COMBOS:
        add("flg/combo/c%dd%dk%d" % (c, d, k), oracle.conduit_compress(data, combo_prefs(c, d, k, W), slice_=300), W)
    # BD
    add("bd/bit7", patched(base, 5, bytes([base[5] | 0x80]), seal=True))
    for b in range(4):
        add("bd/low%d" % b, patched(base, 5, bytes([base[5] | (1 << b)]), seal=True))
    for i in range(4):
        add("bd/bsid%d" % i, patched(base, 5, bytes([i << 4]), seal=True))
    # header checksum, magic
    add("hc/wrong", patched(base, 18, bytes([base[18] ^ 0x5A])))
    add("magic/unknown", patched(base, 0, le32(MAGIC + 1)))
    for k in range(16):
        add("skip/%x/p0" % k, skippable(k, b""))
        add("skip/%x/p11" % k, skippable(k, b"eleven byte"))
    add("skip/cut_size", skippable(3, b"eleven byte")[:6])
    add("skip/cut_size7", skippable(3, b"eleven byte")[:7])
    add("skip/cut_payload", skippable(3, b"eleven byte")[:13])
    add("skip/then_frame", skippable(7, b"eleven byte") + base)
    # size words and the closing words
    p0, _ = blocks_of(base)[0]
    add("word/bs+1/compressed", patched(base, p0, le32(BS + 1)))
    add("word/bs+1/stored", patched(base, p0, le32(0x80000000 | (BS + 1))))
    add("word/stored_bs", stored_full_block_frame(), BS)
    e = end_of_blocks(base)
    assert base[e:e + 4] == bytes(4) and e + 8 == n
    add("end/no_endmark", base[:e])
    add("end/bck_cut", base[:e - 2])
    add("end/bck_wrong", patched(base, e - 4, bytes([base[e - 4] ^ 1])))
    add("end/cck_cut", base[:n - 2])
    add("end/cck_wrong", patched(base, n - 1, bytes([base[n - 1] ^ 0x80])))
    add("csize/+1", patched(base, 6, (W + 1).to_bytes(8, "little"), seal=True))
    add("csize/-1", patched(base, 6, (W - 1).to_bytes(8, "little"), seal=True))
    add("empty/cck0", oracle.conduit_compress(b"", prefs(cck=0)), 0)
    add("empty/cck1", oracle.conduit_compress(b"", prefs(cck=1)), 0)
    # windows
    add("win/exact", base, W)
    add("win/-1", base, W - 1)
    add("win/0", base, 0)
    one = oracle.conduit_compress(data, combo_prefs(1, 1, 1, W))                # the same content as one block
    add("win1/exact", one, W)
    add("win1/-1", one, W - 1)
    add("win1/0", one, 0)
    assert len({name for name, _, _ in out}) == len(out)
    return out


NO_INFO = 99                       # Verdict.info.frameType when the oracle did not get through the header


class Verdict:
    """What the oracle says about the first frame of `frame` decoded into `window` bytes.  `info` is filled once the header
    (or a whole skippable frame) has been accepted, whatever comes after it: header_ok."""
    __slots__ = ("error", "out", "consumed", "info")

    def __init__(self, error, out, consumed, info):
        self.error, self.out, self.consumed, self.info = error, out, consumed, info

    @property
    def header_ok(self):
        return self.info.frameType != NO_INFO


def verdict(frame: bytes, window: int) -> Verdict:
    L = oracle.lib()
    buf = ctypes.create_string_buffer(max(window, 1))
    used, fi = ctypes.c_size_t(0), oracle.FrameInfo()
    fi.frameType = NO_INFO
    src = ctypes.create_string_buffer(bytes(frame), max(len(frame), 1))
    r = L.orc_decompress_frame(src, len(frame), buf, window, ctypes.byref(used), ctypes.byref(fi))
    if L.orc_is_error(r):
        return Verdict(L.orc_error_name(r).decode(), None, 0, fi)
    return Verdict(None, buf.raw[:r], used.value, fi)


ERROR_NAMES = ["OK_NoError", "ERROR_GENERIC", "ERROR_maxBlockSize_invalid", "ERROR_blockMode_invalid", "ERROR_contentChecksumFlag_invalid",
               "ERROR_compressionLevel_invalid", "ERROR_headerVersion_wrong", "ERROR_blockChecksum_invalid", "ERROR_reservedFlag_set",
               "ERROR_allocation_failed", "ERROR_srcSize_tooLarge", "ERROR_dstMaxSize_tooSmall", "ERROR_frameHeader_incomplete",
               "ERROR_frameType_unknown", "ERROR_frameSize_wrong", "ERROR_srcPtr_wrong", "ERROR_decompressionFailed",
               "ERROR_headerChecksum_invalid", "ERROR_contentChecksum_invalid", "ERROR_frameDecoding_alreadyStarted", "ERROR_maxCode"]


def status_of(name) -> int:
    """LZ4F error name (None: no error) -> the status number a result record carries."""
    return 0 if name is None else ERROR_NAMES.index(name)
