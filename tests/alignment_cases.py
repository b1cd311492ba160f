"""The case lists of the alignment tests (test helper, not a test module): tests/test_gpu_alignment.py runs them on the GPU,
tests/test_alignment_cases_cpu.py holds the same lists to the oracle without one, so that a wrong input is found there.

Every device-pointer call takes plain pointers; torch's allocator hands out 512-byte aligned ones, so a suite that never
moves a buffer has only ever seen one alignment.  `carve` makes a view at a chosen byte residue with guard bytes on both
sides INSIDE the allocation (nothing here ever touches an allocation's edge); the lists below say which residues, framings,
finders, inputs and checksum lengths are gone through, and the pairing functions which residues meet."""
from __future__ import annotations

import struct

import numpy as np

PAT = 0xA5
GUARD = 4096


def carve(n: int, mis: int, guard: int = GUARD, device="cpu", align: int = 64):
    """One uint8 tensor of guard + align + n + guard bytes of PAT -> (the view of n bytes that starts `mis` bytes past an
    `align`-byte boundary, the bytes in front of it, the bytes behind it).  Both guards lie inside the allocation and hold at
    least `guard` bytes.  align = 64 unless a residue beyond 63 is asked for (16 + 256 past a 512-byte boundary)."""
    import torch
    assert 0 <= mis < align and align & (align - 1) == 0 and n >= 0
    t = torch.full((guard + align + n + guard,), PAT, dtype=torch.uint8, device=device)
    start = guard + (mis - (t.data_ptr() + guard)) % align
    return t[start:start + n], t[:start], t[start + n:]


def intact(*guards) -> bool:
    return all(bool((g == PAT).all()) for g in guards)


# ---- encode sweep -----------------------------------------------------------------------------------------------------------
# pass E1 shared as it runs by default; the same with runs of 16 tiles per workgroup (below); E1 solo (set_deterministic); the
# hash-chain finder at two levels
FINDERS = ("e1", "e1run", "solo", "hc3", "hc9")
# Pass E1 loads a workgroup's first tile and a short last tile byte-wise (e1_fill) and every other tile by LDS-DMA (e1_dma_piece).
# A workgroup takes n_tiles / CUs tiles (engine.hip: encode_plan), so on a 256-CU device an input under 32 MiB has one tile
# per workgroup and NEVER reaches the DMA loader.  "e1run" makes the engine with this switch - the runs inputs of 256 MiB and
# more get by themselves - so that the 9 MiB input goes through the DMA for 15 tiles of 16 at every residue; BIG_E1 are
# placements of an input big enough to get there without the switch.
E1_RUN_ENV = {"LZ4F_MI355X_E1_RUN": "16"}
BIG_E1 = [("indep4m_bck", 1, 0), ("linked64k", 6, 3), ("indep64k", 11, 13), ("linked4m_cck", 15, 1)]     # (framing, source residue, frame residue)


def big_input() -> bytes:
    from lz4_frame_conduit_amd import datagen
    return datagen.synth50(48 << 20, 93)[:(48 << 20) - 54321].tobytes()
SRC_RES = list(range(16)) + [17, 31, 33, 63]
DST_RES = [0, 1, 3, 8, 13]
TABLE_RES = [8, 24]                                        # block tables hold 64-bit words: natural alignment, not 16
INDEX_RES = [(16, 64), (48, 64), (16 + 256, 512)]          # (residue, boundary): sequence indexes hold 16-byte units
# (blockSizeID, independent, block checksum, content checksum)
FRAMINGS = {"indep64k": (4, 1, 0, 0), "linked64k": (4, 0, 0, 0), "indep4m_bck": (7, 1, 1, 0), "linked4m_cck": (7, 0, 0, 1)}
INDEP, LINKED = ("indep64k", "indep4m_bck"), ("linked64k", "linked4m_cck")
TINY = [(b"abcab" * 8)[:n] for n in range(34)]


def inputs():
    """name -> bytes.  synth50: many full 64 KiB tiles per workgroup (pass E1's DMA loader) and a short last tile (its per-byte
    loader); text: the dense path; a short period; and lengths around the format's smallest blocks."""
    from lz4_frame_conduit_amd import datagen
    out = {"synth50": datagen.synth50(9 << 20, 92)[:(9 << 20) - 12345].tobytes(),
           "text": datagen.synth_text((2 << 20) + 1024, 17)[:(2 << 20) + 777].tobytes(),
           "period3": (b"abc" * 100000)[:300000]}
    for n, t in enumerate(TINY):
        out["tiny%d" % n] = t
    return out


def encode_cases():
    """[(finder, input name, framing name, source residue, frame residue, table residue)].  Per finder and source residue: synth50
    in one independent and one linked framing; text and period3 in one framing each (independent and linked by turns); the
    tiny lengths go round the residues and framings.  Frame residues go round DST_RES, table residues round TABLE_RES."""
    out, k = [], 0
    for fi, finder in enumerate(FINDERS):
        for ri, s in enumerate(SRC_RES):
            a, b = INDEP[(ri // 2 + fi) % 2], LINKED[(ri // 2 + fi) % 2]
            for name, fr in (("synth50", a), ("synth50", b), ("text", b if ri % 2 else a), ("period3", a if ri % 2 else b)):
                out.append((finder, name, fr, s, DST_RES[k % len(DST_RES)], TABLE_RES[k % 2])); k += 1
        for n in range(len(TINY)):
            fr = list(FRAMINGS)[(n + fi) % 4]
            out.append((finder, "tiny%d" % n, fr, SRC_RES[(n + 3 * fi) % len(SRC_RES)], DST_RES[k % len(DST_RES)], TABLE_RES[k % 2])); k += 1
    return out


def index_cases():
    """[(finder, input name, framing name, source residue, frame residue, table residue, (index residue, boundary))]: every index
    placement with every table placement, in every framing."""
    out, k = [], 0
    for ix in INDEX_RES:
        for tb in TABLE_RES:
            for fr in FRAMINGS:
                for name in ("synth50", "text"):
                    out.append((FINDERS[k % len(FINDERS)], name, fr, SRC_RES[(5 * k + 1) % len(SRC_RES)], DST_RES[k % len(DST_RES)], tb, ix)); k += 1
    return out


# ---- decode sweep -----------------------------------------------------------------------------------------------------------
RES16 = list(range(16))


def dst_for(frame_res: int, turn: int = 0) -> int:
    """The destination residue a frame residue is paired with: a bijection of 0..15 for every `turn` (7 is odd), another per turn."""
    return (7 * frame_res + 5 + 3 * turn) % 16


def frame_for(dst_res: int, turn: int = 0) -> int:
    """The frame residue a destination residue is paired with (the grammar subset goes by destination residues)."""
    return (11 * dst_res + 2 + 5 * turn) % 16


# one accepted and one rejected case of each family of lz4_grammar.corpus() (mext and lext have no rejected case: every extension
# they write is valid); small frames, so that every switch set can meet every destination residue
GRAMMAR_SUBSET = {
    "end": ("end/dense/full/M8/k5", "end/dense/full/M8/k4"),
    "lit": ("lit/mid/L270", "lit/cut/short_by_one"),
    "off": ("off/reach/mid/L4/+0", "off/reach/mid/L4/+1"),
    "mext": ("mext/align3", None),
    "lext": ("lext/align5", None),
    "link": ("link/bsid4/hist_1000+3000+7/+0", "link/bsid4/hist_1000+3000+7/+1"),
    "blk": ("blk/indep/short_mid/bck1_cck1", "blk/stored_bs/bsid4/+1"),
    "carrier": ("carrier/linked4/dense/k5", "carrier/indep4/sparse/k4"),
}
# liblz4 1.9.3 has two names for a block that does not decode, by the room it had (tests/test_oracle_grammar.py); a decoder
# that gives either has given liblz4's verdict
BLOCK_FAILED = ("ERROR_GENERIC", "ERROR_decompressionFailed")


def same_verdict(got: str, recorded: str) -> bool:
    return got == recorded or (got in BLOCK_FAILED and recorded in BLOCK_FAILED)


# ---- checksum sweep ---------------------------------------------------------------------------------------------------------
# on the seams of lane4_xxh32's loop: 16-byte stripes, 1 KiB steps (64 stripes), rounds of four steps (4 KiB), the tail
XXH_LENS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 1007, 1008, 1023, 1024, 1025, 1039, 1040, 4095, 4096, 4097, 4111, 4112,
            8191, 8192, 8193, 65535, 65536, 100001, 1 << 20, (4 << 20) - 1]
XXH_RES = 4                                                # placements per length (the counters ask for at least four)
MANY_BLOCKS = 16384 + 3                                    # from XXH_LANE4_BELOW blocks on the scalar form of the block checksum runs


def _rng_bytes(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def checksum_frames():
    """[(name, frame, content, [offset of each block checksum], offset of the content checksum)]: hand-built frames of stored
    blocks with block and content checksums.  One frame per length (one block: the content checksum runs over the same
    length); the lengths of 64 KiB and less together in one 64 KiB-block frame; all of them together in one 4 MiB-block frame."""
    from lz4_grammar import Frame
    out = []

    def build(name, bsid, lens, seed):
        fr = Frame(bsid, bck=True, cck=True)
        at, pos = [], 7
        for k, n in enumerate(lens):
            if n == 0:
                continue                                   # (a block of no bytes is the EndMark: length 0 is the frame without blocks)
            fr.stored(_rng_bytes(seed + k, n))
            pos += 4 + n; at.append(pos); pos += 4
        fb = fr.bytes()
        assert pos + 8 == len(fb)
        out.append((name, fb, bytes(fr.out), at, len(fb) - 4))

    for n in XXH_LENS:
        build("one/%d" % n, 4 if n <= 65536 else 7, [n] if n else [], 1000 + n % 977)
    build("all/64k", 4, [n for n in XXH_LENS if n <= 65536], 5)
    build("all/4m", 7, XXH_LENS, 6)
    return out


def flip(frame: bytes, at: int, bit: int = 0) -> bytes:
    b = bytearray(frame); b[at] ^= 1 << bit
    return bytes(b)


def checksum_placements(k: int):
    """The XXH_RES (frame residue, destination residue) pairs of the k-th checksum frame; over the frames every residue 0..15 comes
    up on both sides (k and k + 1 are sixteen placements apart in steps of four)."""
    return [((k + 4 * j) % 16, (3 * k + 4 * j + 1) % 16) for j in range(XXH_RES)]


def many_blocks_frame():
    """A frame of MANY_BLOCKS stored blocks of 1..64 KiB with block checksums (about 0.5 GiB) as a numpy array, its content, and the
    (payload offset, length) of every block.  Built with numpy, checksums by the oracle."""
    import oracle
    from lz4_grammar import Frame
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 65537, MANY_BLOCKS)
    lens[:4] = (65536, 1, 1024, 4112)
    content = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    hdr = Frame(4, bck=True).header()
    frame = np.empty(len(hdr) + int(lens.sum()) + 8 * MANY_BLOCKS + 4, dtype=np.uint8)
    frame[:len(hdr)] = np.frombuffer(hdr, dtype=np.uint8)
    pos, src, blocks = len(hdr), 0, []
    for n in lens.tolist():
        frame[pos:pos + 4] = np.frombuffer(struct.pack("<I", n | 0x80000000), dtype=np.uint8)
        frame[pos + 4:pos + 4 + n] = content[src:src + n]
        frame[pos + 4 + n:pos + 8 + n] = np.frombuffer(struct.pack("<I", oracle.xxh32(content[src:src + n])), dtype=np.uint8)
        blocks.append((pos + 4, n)); pos += 8 + n; src += n
    frame[pos:pos + 4] = 0
    assert pos + 4 == len(frame)
    return frame, content, blocks


def walk(frame) -> "tuple[list, int]":
    """The blocks of a well-formed frame: [(payload offset, size word)], and the position behind the EndMark."""
    flg = int(frame[4])
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    blocks = []
    while True:
        w = int.from_bytes(bytes(frame[pos:pos + 4]), "little"); pos += 4
        if w == 0:
            return blocks, pos
        blocks.append((pos, w)); pos += (w & 0x7FFFFFFF) + 4 * ((flg >> 4) & 1)
