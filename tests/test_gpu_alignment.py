"""The device-pointer calls on buffers at every byte alignment.

torch's allocator hands out 512-byte aligned memory, so the rest of the suite only ever gave lz4f_mi355x_dev_* sources, frames,
destinations, tables and indexes that start on such a boundary; include/lz4f_mi355x.h takes plain pointers (its alignment
contract: data buffers any byte address, block tables 8 bytes, sequence indexes 16, the in-band frame buffer 16).  Here every
buffer a call reads or writes is carved (tests/alignment_cases.py) at a chosen residue out of a bigger allocation, with guard
bytes on both sides inside it that must come back untouched.  The reference of every comparison is the CPU oracle and the
input bytes themselves; tests/test_alignment_cases_cpu.py holds the same case lists to the oracle without a GPU.

The last test asserts the coverage the others recorded (run the whole file)."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import oracle
import alignment_cases as ac
from alignment_cases import carve, intact
from conftest import GOLDEN_DIR
from lz4_frame_conduit_amd import _ffi, conduit
from lz4_frame_conduit_amd.device import DeviceCodecError, Engine
from lz4_grammar import corpus
from test_gpu_batch_frames import assert_same, oracle_out, single
from test_gpu_grammar import ENVS, _walk as walk_or_none
from test_gpu_parity import PATH, RATIO_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sha = lambda b: hashlib.sha256(b).hexdigest()
IX_MAGIC = 0x3258494C
BLOCK_DT = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("word", "<u4"), ("dst_size", "<u4")])

# what the sweeps reached (test_coverage_reached, at the end)
COVER = dict(enc=set(), env_dst=set(), dec=set(), xxh_blocks=collections.defaultdict(set), xxh_content=collections.defaultdict(set),
             xxh_write_blocks=collections.defaultdict(set), xxh_write_content=collections.defaultdict(set), many=set())


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    return ac.inputs()


@pytest.fixture(scope="module")
def on_dev(inputs):
    return {k: dev(v) for k, v in inputs.items()}


@pytest.fixture(scope="module")
def oracle_frames(inputs):
    """(input name, framing name) -> the oracle's (= liblz4's) frame."""
    out = {}
    for name, data in inputs.items():
        for fr, (bsid, indep, bck, cck) in ac.FRAMINGS.items():
            out[name, fr] = oracle.conduit_compress(data, oracle.mkprefs(bsid=bsid, indep=indep, bck=bck, cck=cck))
    return out


def dev(b) -> torch.Tensor:
    a = np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b
    return torch.from_numpy(a.copy()).to(DEV) if len(a) else torch.zeros(0, dtype=torch.uint8, device=DEV)


def place(t: torch.Tensor, mis: int, align: int = 64, room: int = 0):
    """A copy of device tensor t carved at residue mis (room: at least that many bytes, the rest PAT): (view, front, back)."""
    v, f, b = carve(max(t.numel(), room), mis, device=DEV, align=align)
    v[:t.numel()].copy_(t)
    return v, f, b


def prefs_for(framing: str, level: int = 0):
    bsid, indep, bck, cck = ac.FRAMINGS[framing]
    return conduit.make_preferences(blockSizeID=bsid, blockMode=indep, contentChecksum=cck, blockChecksum=bck, compressionLevel=level)


def table_of(frame: bytes, content: int, bs: int) -> np.ndarray:
    """The caller's block table of a well-formed frame, as the walk kernel writes it: block i at i * maxBlockSize."""
    blocks, _ = ac.walk(frame)
    ent = np.zeros(len(blocks) + 1, dtype=BLOCK_DT)
    for i, (p, w) in enumerate(blocks):
        ent[i] = (p, i * bs, w, min(bs, max(content - i * bs, 0)))
    return ent


def err_name(e: Exception) -> str:
    return str(e).split(" ")[0]


# ---- encode: source, frame, table and index moved -------------------------------------------------------------------------------
def encode_one(eng, data: bytes, data_dev, p, s_res, d_res, t_res, ix=None, where=None):
    """One compress call on carved buffers; everything the issue asks of a case but the comparison between placements.
    -> (the frame's bytes, the result record)."""
    n, bs = len(data), 1 << (8 + 2 * p.frameInfo.blockSizeID)
    nb = -(-n // bs)
    src, sf, sb = place(data_dev, s_res)
    dst, df, db = carve(eng.frame_bound(n, p), d_res, device=DEV)
    tbl, tf, tb = carve((nb + 1) * BLOCK_DT.itemsize, t_res, device=DEV); tbl.zero_()
    guards = [sf, sb, df, db, tf, tb]
    index = None
    if ix is not None:
        index, xf, xb = carve(eng.index_size(n, p), ix[0], device=DEV, align=ix[1]); index.zero_()
        guards += [xf, xb]
    eng.compress_async(src, dst, p, tbl, index)
    r = eng.result()
    assert 0 < r.size <= dst.numel(), where
    host = dst[:r.size].cpu().numpy().tobytes()
    out, used = oracle.decompress_frame(host, cap=n + 64)                     # the oracle decodes what the GPU wrote
    assert used == r.size and out == data, where
    # the record and the block table are true: every entry's size word is the frame's, every block at its place
    blocks, end = ac.walk(host)
    assert r.n_blocks == nb == len(blocks) and end + 4 * p.frameInfo.contentChecksumFlag == r.size, where
    ent = np.frombuffer(tbl.cpu().numpy().tobytes(), dtype=BLOCK_DT)[:nb]
    assert [(int(e["src_off"]), int(e["word"])) for e in ent] == blocks, where
    assert [(int(e["dst_off"]), int(e["dst_size"])) for e in ent] == [(i * bs, min(bs, n - i * bs)) for i in range(nb)], where
    # the device decoder gives the input back (the destination moved too)
    back, bf, bb = carve(max(n, 1), ac.dst_for(s_res % 16, d_res), device=DEV)
    guards += [bf, bb]
    eng.decompress_frame_async(dst, int(r.size), back)
    r2 = eng.result()
    assert r2.size == n and r2.consumed == r.size and torch.equal(back[:n], data_dev), where
    if index is not None:                                                     # and by the index this call left
        hd = index[:32].cpu().numpy().view(np.uint32)
        back.fill_(ac.PAT)
        eng.decompress_blocks_async(dst, int(r.size), back, tbl, nb, p.frameInfo, index)
        r3 = eng.result()
        assert r3.size == n and torch.equal(back[:n], data_dev), where
        if hd[0] == IX_MAGIC and hd[3] > 0 and (p.frameInfo.blockSizeID >= 5 or not p.frameInfo.blockMode):
            path = int(r3.flags) >> 12                                        # (as test_indexed_decode_same_bytes_as_generic expects it)
            assert path & PATH["indexed"] and not path & PATH["dropped"], (where, hex(path))
    assert torch.equal(src, data_dev) and intact(*guards), where
    return host, r


@pytest.mark.parametrize("finder", ac.FINDERS)
def test_encode_source_and_frame_moved(inputs, on_dev, oracle_frames, finder):
    if finder == "e1run": os.environ.update(ac.E1_RUN_ENV)                   # (switches are read when an engine is made)
    try:
        eng = Engine(0)
    finally:
        for k in ac.E1_RUN_ENV: os.environ.pop(k, None)
    if finder == "solo": eng.set_deterministic(True)
    level = {"hc3": 3, "hc9": 9}.get(finder, 0)
    ref = {}                                                                  # (input, framing) -> the frame at misalignment 0
    cases = [c + (None,) for c in ac.encode_cases() if c[0] == finder] + [c for c in ac.index_cases() if c[0] == finder]
    for _, name, fr, s_res, d_res, t_res, ix in cases:
        p = prefs_for(fr, level)
        where = (finder, name, fr, s_res, d_res, t_res, ix)
        frame, r = encode_one(eng, inputs[name], on_dev[name], p, s_res, d_res, t_res, ix, where)
        if finder in ("e1", "e1run"):
            # the shared search is timing-dependent: its frames are held to liblz4's size, the bar of test_compress_roundtrip_and_ratio
            if name in ("synth50", "text"):
                assert len(frame) <= len(oracle_frames[name, fr]) * RATIO_TOL, (where, len(frame), len(oracle_frames[name, fr]))
        else:
            # solo and hash-chain frames are a function of the input alone: byte-identical to the frame at misalignment 0
            if (name, fr) not in ref:
                ref[name, fr] = sha(encode_one(eng, inputs[name], on_dev[name], p, 0, 0, 8, None, where + ("aligned",))[0])
            assert sha(frame) == ref[name, fr], where
        COVER["enc"].add((finder, s_res))
    if finder == "e1":                                                        # an input with several tiles per workgroup by itself
        big = ac.big_input()
        big_dev = dev(big)
        for fr, s_res, d_res in ac.BIG_E1:
            bsid, indep, bck, cck = ac.FRAMINGS[fr]
            where = (finder, "big", fr, s_res, d_res)
            frame, r = encode_one(eng, big, big_dev, prefs_for(fr), s_res, d_res, 8, None, where)
            ref_len = len(oracle.conduit_compress(big, oracle.mkprefs(bsid=bsid, indep=indep, bck=bck, cck=cck)))
            assert len(frame) <= ref_len * RATIO_TOL, (where, len(frame), ref_len)
    eng.close()


def test_inband_refuses_a_misaligned_frame_buffer(eng, inputs, on_dev):
    """The one alignment the encoder asks for: the in-band trailer's frame buffer (16 bytes).  Refused by name, nothing written."""
    p = prefs_for("indep4m_bck")
    for res in (1, 4, 8):
        dst, df, db = carve(eng.frame_bound_inband(len(inputs["text"]), p), res, device=DEV)
        with pytest.raises(DeviceCodecError, match="ERROR_GENERIC.*16-byte aligned"):
            eng.compress_async(on_dev["text"], dst, p, inband=True)
        torch.cuda.synchronize()
        assert intact(df, db, dst)


# ---- decode: frame and destination moved ------------------------------------------------------------------------------------------
def decode_frame(eng, f_dev, flen, n, f_res, d_res):
    """decompress_frame_async on carved buffers -> (record or error name, the destination view); guards checked."""
    fr, ff, fb = place(f_dev, f_res)
    back, bf, bb = carve(max(n, 1), d_res, device=DEV)
    try:
        eng.decompress_frame_async(fr, flen, back); r = eng.result()
    except DeviceCodecError as e:
        r = err_name(e)
    torch.cuda.synchronize()
    assert intact(ff, fb, bf, bb) and torch.equal(fr[:f_dev.numel()], f_dev), (f_res, d_res)
    return r, back


def decode_table(eng, f_dev, flen, n, ent, info, f_res, d_res, t_res, index=None, ix=None, cap=None):
    fr, ff, fb = place(f_dev, f_res)
    back, bf, bb = carve(max(n, 1) if cap is None else cap, d_res, device=DEV)
    tbl, tf, tb = place(dev(ent.tobytes()), t_res)
    guards = [ff, fb, bf, bb, tf, tb]
    if index is not None:
        index, xf, xb = place(index, ix[0], ix[1]); guards += [xf, xb]
    try:
        eng.decompress_blocks_async(fr, flen, back, tbl, len(ent) - 1, info, index); r = eng.result()
    except DeviceCodecError as e:
        r = err_name(e)
    torch.cuda.synchronize()
    assert intact(*guards), (f_res, d_res, t_res, ix)
    return r, back


def test_decode_oracle_frames_moved(eng, inputs, on_dev, oracle_frames):
    turn = 0
    for (name, fr), f in oracle_frames.items():
        data, data_dev, p = inputs[name], on_dev[name], prefs_for(fr)
        n, bs = len(data), 1 << (8 + 2 * p.frameInfo.blockSizeID)
        f_dev, ent = dev(f), table_of(f, len(data), bs)
        tiny = name.startswith("tiny")
        turn += 1
        for f_res in ([(turn + int(name[4:])) % 16] if tiny else ac.RES16):   # (the tiny lengths go round the residues)
            d_res = ac.dst_for(f_res, turn)
            r, back = decode_frame(eng, f_dev, len(f), n, f_res, d_res)
            assert not isinstance(r, str) and (r.size, r.consumed, r.n_blocks) == (n, len(f), len(ent) - 1), (name, fr, f_res, r)
            assert torch.equal(back[:n], data_dev), (name, fr, f_res, d_res)
            COVER["dec"].add(("frame", f_res, d_res))
            if len(ent) == 1:
                continue                                                      # (the frame of no bytes has no blocks to list)
            r, back = decode_table(eng, f_dev, len(f), n, ent, p.frameInfo, f_res, d_res, ac.TABLE_RES[f_res % 2])
            assert not isinstance(r, str) and r.size == n and torch.equal(back[:n], data_dev), (name, fr, f_res, d_res, r)
            assert (int(r.flags) >> 12) & PATH["table"]
            COVER["dec"].add(("blocks", f_res, d_res))


def test_decode_by_index_moved(eng, inputs, on_dev):
    """decompress_blocks_async with the compressor's sequence index: frame, destination, table and index all moved."""
    for k, (name, fr) in enumerate([("synth50", "indep4m_bck"), ("synth50", "linked64k"), ("text", "linked4m_cck"), ("period3", "indep64k")]):
        data_dev, p = on_dev[name], prefs_for(fr)
        n, bs = data_dev.numel(), 1 << (8 + 2 * p.frameInfo.blockSizeID)
        nb = -(-n // bs)
        frame = torch.empty(eng.frame_bound(n, p), dtype=torch.uint8, device=DEV)
        table, index = eng.new_table(nb), eng.new_index(n, p)
        eng.compress_async(data_dev, frame, p, table, index)
        r = eng.result()
        host = frame[:r.size].cpu().numpy().tobytes()
        assert oracle.decompress_frame(host, cap=n + 64) == (inputs[name], r.size)
        ent = np.frombuffer(table.cpu().numpy().tobytes(), dtype=BLOCK_DT)
        hd = index[:32].cpu().numpy().view(np.uint32)
        for f_res in ac.RES16:
            d_res, ix = ac.dst_for(f_res, k), ac.INDEX_RES[(f_res + k) % 3]
            r2, back = decode_table(eng, frame[:r.size], int(r.size), n, ent, p.frameInfo, f_res, d_res, ac.TABLE_RES[(f_res + k) % 2], index, ix)
            assert not isinstance(r2, str) and r2.size == n and torch.equal(back[:n], data_dev), (name, fr, f_res, d_res, r2)
            if hd[0] == IX_MAGIC and hd[3] > 0 and (p.frameInfo.blockSizeID >= 5 or not p.frameInfo.blockMode):
                path = int(r2.flags) >> 12
                assert path & PATH["indexed"] and not path & PATH["dropped"], (name, fr, f_res, hex(path))
                COVER["dec"].add(("blocks_indexed", f_res, d_res))


def test_decode_inband_frames_moved(eng, inputs, on_dev):
    """This library's in-band frames: the trailer is read when the frame starts 16-byte aligned (the header calls it a hint), and
    the bytes are the same wherever it starts."""
    for k, (name, fr) in enumerate([("synth50", "indep4m_bck"), ("synth50", "linked64k"), ("text", "indep64k")]):
        data_dev, p = on_dev[name], prefs_for(fr)
        n = data_dev.numel()
        frame, ff, fb = carve(eng.frame_bound_inband(n, p), 16, device=DEV)      # (16-byte aligned is all the call asks for)
        eng.compress_async(data_dev, frame, p, inband=True)
        r = eng.result()
        assert intact(ff, fb)
        stream = frame[:r.size].cpu().numpy().tobytes()
        out, used = oracle.decompress_frame(stream, cap=n + 64)
        assert out == inputs[name] and used < len(stream), (name, fr)
        for f_res in ac.RES16:
            d_res = ac.dst_for(f_res, k)
            r2, back = decode_frame(eng, frame[:r.size], int(r.size), n, f_res, d_res)
            assert not isinstance(r2, str) and (r2.size, r2.consumed) == (n, used) and torch.equal(back[:n], data_dev), (name, fr, f_res, d_res, r2)
            path = int(r2.flags) >> 12
            if f_res == 0:
                assert path & PATH["trailer"] and not path & PATH["dropped"], (name, fr, hex(path))
            COVER["dec"].add(("inband", f_res, d_res))


@pytest.fixture(scope="module")
def grammar_subset():
    with open(os.path.join(GOLDEN_DIR, "grammar.json")) as f:
        g = json.load(f)["cases"]
    cmap = {n: (f, m) for n, f, m in corpus()}
    out = []
    for fam, pair in ac.GRAMMAR_SUBSET.items():
        for name in pair:
            if name is not None:
                f, m = cmap[name]
                out.append((name, f, m, g[name]["once"]))
    return out


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=["+".join(k[len("LZ4F_MI355X_"):] + ("=" + v if v != "1" else "") for k, v in e.items()) or "default" for e in ENVS])
def test_grammar_subset_under_every_switch_set(grammar_subset, ei):
    """One accepted and one rejected case of each grammar family, under every switch set that changes the decoder, at every
    destination residue: liblz4's bytes and bytes consumed, or liblz4's verdict."""
    L = _ffi.lib()
    env = ENVS[ei]
    os.environ.update(env)
    L.lz4f_mi355x_release_engines()
    try:
        eng = Engine(0)
        for ci, (name, f, meta, once) in enumerate(grammar_subset):
            f_dev = dev(f)
            blocks, end = walk_or_none(f)
            cap = max(len(blocks), 1) * meta["bs"]                           # every block's full room (tests/test_gpu_grammar.py)
            info = _ffi.FrameInfo()
            info.blockSizeID, info.blockMode, info.blockChecksumFlag = (f[5] >> 4) & 7, (f[4] >> 5) & 1, (f[4] >> 4) & 1
            ent = np.zeros(len(blocks) + 1, dtype=BLOCK_DT)
            for i, (pp, w) in enumerate(blocks):
                ent[i] = (pp, i * meta["bs"], w, meta["bs"])
            for d_res in ac.RES16:
                f_res = ac.frame_for(d_res, ci + ei)
                calls = [("frame", decode_frame(eng, f_dev, len(f), cap, f_res, d_res))]
                if end is not None:
                    calls.append(("table", decode_table(eng, f_dev, len(f), 0, ent, info, f_res, d_res, ac.TABLE_RES[d_res % 2], cap=cap)))
                for entry, (r, back) in calls:
                    where = (env, name, entry, f_res, d_res, r if isinstance(r, str) else None)
                    if once["error"] is None:
                        assert not isinstance(r, str) and r.size == meta["content"], where
                        assert sha(back[:r.size].cpu().numpy().tobytes()) == once["out_sha256"], where
                        if entry == "frame": assert r.consumed == once["consumed"] == len(f), where
                    else:
                        assert isinstance(r, str) and ac.same_verdict(r, once["error"]), where
                COVER["env_dst"].add((ei, d_res))
                COVER["dec"].add(("frame", f_res, d_res))
        eng.close()
    finally:
        for k in env: os.environ.pop(k, None)
        L.lz4f_mi355x_release_engines()


def test_batch_offsets_at_every_residue(eng, inputs, oracle_frames, grammar_subset):
    """64 small frames in one batch call, placed so that src_off[i] % 16 and dst_off[i] % 16 each take every value (and both
    buffers start off a boundary themselves); each frame as the single call decodes it and as the oracle does."""
    fs = [("tiny%d/%s" % (n, fr), oracle_frames["tiny%d" % n, fr]) for n in range(34) for fr in (list(ac.FRAMINGS)[n % 4],)]
    fs += [(name, f) for name, f, _, _ in grammar_subset if len(f) < (128 << 10)]
    small = inputs["text"][:70000]
    for k in range(64 - len(fs)):
        bsid, indep, bck, cck = list(ac.FRAMINGS.values())[k % 4]
        fs.append(("made%d" % k, oracle.conduit_compress(small[k * 1000:k * 1000 + 3000 + 2000 * k], oracle.mkprefs(bsid=4, indep=indep, bck=bck | (k & 1), cck=cck))))
    fs = fs[:64]
    assert len(fs) == 64
    outs = [oracle_out(f) for _, f in fs]
    caps = [(len(o) if o is not None else 4 * len(f) + 64) + (0, 17, 1 << 16)[i % 3] for i, ((_, f), o) in enumerate(zip(fs, outs))]
    G = 192
    so, do, real = [0], [0], []
    for i, ((_, f), c) in enumerate(zip(fs, caps)):
        rs, rd = i % 16, (5 * i + 3) % 16
        assert so[-1] % 16 == rs
        gap = G + (rd - (do[-1] + G)) % 16
        so.append(so[-1]); do.append(do[-1] + gap)                            # the guard in front: an empty span, its window the gap
        real.append(len(so) - 1)
        pad = ((i + 1) % 16 - (so[-1] + len(f))) % 16                         # (the next span's residue: padding behind this frame)
        so.append(so[-1] + len(f) + pad); do.append(do[-1] + c)
    so.append(so[-1]); do.append(do[-1] + G)
    assert {so[k] % 16 for k in real} == {do[k] % 16 for k in real} == set(range(16))
    blob = bytearray(so[-1])
    for (_, f), k in zip(fs, real):
        blob[so[k]:so[k] + len(f)] = f
    src, sf, sb = place(dev(bytes(blob)), 5)
    dst, df, db = carve(do[-1], 11, device=DEV)
    res = eng.new_results(len(so) - 1)
    eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device=DEV), dst, torch.tensor(do, dtype=torch.int64, device=DEV), res)
    recs = eng.frame_results(res)
    out = dst.cpu().numpy().tobytes()
    assert intact(sf, sb, df, db)
    n_ok = 0
    for k in range(len(recs)):
        if k not in set(real):
            assert recs[k].status == 12 and out[do[k]:do[k + 1]] == bytes([ac.PAT]) * (do[k + 1] - do[k]), k
    for i, ((name, f), cap, k) in enumerate(zip(fs, caps, real)):
        want, wout = single(eng, f, cap)
        assert_same(recs[k], want, name)
        if recs[k].status == 0:
            n_ok += 1
            got = out[do[k]:do[k] + recs[k].size]
            assert got == wout and outs[i] is not None and got == outs[i], name
        else:                                                                 # (11: a short block in the middle needs every block's full room)
            assert outs[i] is None or recs[k].status == 11, (name, recs[k].status)
        COVER["dec"].add(("frames", (5 + so[k]) % 16, (11 + do[k]) % 16))
    assert n_ok > 40


# ---- the checksum kernels the codec runs ---------------------------------------------------------------------------------------------
def test_checksums_verified_at_every_seam(eng):
    """Hand-built frames of stored blocks whose lengths sit on the seams of lane4_xxh32's loop, at four placements each: accepted;
    rejected by name with one bit of a block checksum, or of the content checksum, flipped."""
    for k, (name, f, content, bck_at, cck_at) in enumerate(ac.checksum_frames()):
        n, c_dev = len(content), dev(content)
        blocks, _ = ac.walk(f)
        # (blocks shorter than maxBlockSize in the middle: the call decodes block i at i * maxBlockSize, so it needs every block's full room)
        cap = n if len(blocks) <= 1 else len(blocks) << (8 + 2 * ((f[5] >> 4) & 7))
        for j, (f_res, d_res) in enumerate(ac.checksum_placements(k)):
            where = (name, f_res, d_res)
            r, back = decode_frame(eng, dev(f), len(f), cap, f_res, d_res)
            assert not isinstance(r, str) and (r.size, r.consumed, r.n_blocks) == (n, len(f), len(blocks)), (where, r)
            assert torch.equal(back[:n], c_dev), where
            if bck_at:
                b = (k + j) % len(bck_at)
                r, _ = decode_frame(eng, dev(ac.flip(f, bck_at[b] + (k + j) % 4, (3 * k + j) % 8)), len(f), cap, f_res, d_res)
                assert r == "ERROR_blockChecksum_invalid", (where, b, r)
            r, _ = decode_frame(eng, dev(ac.flip(f, cck_at + (k + j) % 4, (5 * k + j) % 8)), len(f), cap, f_res, d_res)
            assert r == "ERROR_contentChecksum_invalid", (where, r)
            for p, w in blocks:
                COVER["xxh_blocks"][w & 0x7FFFFFFF].add((f_res + p) % 16)
            COVER["xxh_content"][n].add(d_res)


def test_checksums_written_at_every_seam(eng):
    """The write side: random bytes of the same lengths come out as stored blocks; the checksum words in the frame are the
    oracle's XXH32 of each payload and of the input."""
    for k, n in enumerate(ac.XXH_LENS):
        data = np.random.default_rng(4000 + k).integers(0, 256, n, dtype=np.uint8).tobytes()
        d_dev = dev(data)
        p = conduit.make_preferences(blockSizeID=4 if n <= 65536 else 7, blockMode=1, contentChecksum=1, blockChecksum=1)
        bs = 1 << (8 + 2 * p.frameInfo.blockSizeID)
        for s_res, d_res in ac.checksum_placements(k):
            src, sf, sb = place(d_dev, s_res)
            dst, df, db = carve(eng.frame_bound(n, p), d_res, device=DEV)
            eng.compress_async(src, dst, p)
            r = eng.result()
            f = dst[:r.size].cpu().numpy().tobytes()
            assert intact(sf, sb, df, db), (n, s_res, d_res)
            blocks, end = ac.walk(f)
            assert end + 4 == len(f) and len(blocks) == -(-n // bs) == r.n_blocks, (n, s_res, d_res)
            pos = 0
            for pp, w in blocks:
                ln = w & 0x7FFFFFFF
                assert w >> 31 and f[pp:pp + ln] == data[pos:pos + ln], (n, s_res, d_res)              # stored
                assert int.from_bytes(f[pp + ln:pp + ln + 4], "little") == oracle.xxh32(data[pos:pos + ln]), (n, s_res, d_res, pos)
                COVER["xxh_write_blocks"][ln].add((d_res + pp) % 16)
                pos += ln
            assert pos == n and int.from_bytes(f[-4:], "little") == oracle.xxh32(data), (n, s_res, d_res)
            COVER["xxh_write_content"][n].add(s_res)


def test_checksums_of_many_blocks(eng):
    """From 16384 blocks on the block checksums are computed a wave per block on the scalar unit (k_xxh32_blocks), not by
    lane4_xxh32: a frame of 16384 + 3 stored blocks carved at residue 5 is verified, and as many blocks are written."""
    LIMIT = 16384                                                             # XXH_LANE4_BELOW (csrc/frame_dev.cuh)
    frame, content, blocks = ac.many_blocks_frame()
    assert len(blocks) == ac.MANY_BLOCKS >= LIMIT
    fr, ff, fb = carve(len(frame), 5, device=DEV)
    fr.copy_(torch.from_numpy(frame))
    cap = ac.MANY_BLOCKS << 16                                                # every block's full room: the decoder's block bound is then >= the count
    assert cap // 65536 + 2 >= LIMIT
    back, bf, bb = carve(cap, 11, device=DEV)
    c_dev = torch.from_numpy(content).to(DEV)
    eng.decompress_frame_async(fr, len(frame), back)
    r = eng.result()
    assert (r.size, r.consumed, r.n_blocks) == (len(content), len(frame), ac.MANY_BLOCKS)
    assert torch.equal(back[:len(content)], c_dev) and intact(ff, fb, bf, bb)
    p0, n0 = blocks[ac.MANY_BLOCKS - 2]                                        # one bit of one checksum word
    fr[p0 + n0 + 2] ^= 0x20
    with pytest.raises(DeviceCodecError, match="ERROR_blockChecksum_invalid"):
        eng.decompress_frame_async(fr, len(frame), back); eng.result()
    assert intact(ff, fb, bf, bb)
    COVER["many"].add("verify")
    del back, bf, bb, fr, ff, fb
    # the write side: as many blocks of random bytes (64 KiB each, stored), source carved at residue 5
    n = (ac.MANY_BLOCKS << 16) - 777
    src, sf, sb = carve(n, 5, device=DEV)
    src.copy_(c_dev.repeat(3)[:n])
    p = conduit.make_preferences(blockSizeID=4, blockMode=1, blockChecksum=1)
    dst, df, db = carve(eng.frame_bound(n, p), 3, device=DEV)
    eng.compress_async(src, dst, p)
    r = eng.result()
    assert r.n_blocks == ac.MANY_BLOCKS >= LIMIT and intact(sf, sb, df, db)
    f = dst[:r.size].cpu().numpy()
    data = np.tile(content, 3)[:n]
    wb, end = ac.walk(f)
    assert end == len(f) and len(wb) == ac.MANY_BLOCKS
    pos = 0
    for pp, w in wb:
        ln = w & 0x7FFFFFFF
        assert w >> 31 and ln == min(65536, n - pos)
        assert int.from_bytes(f[pp + ln:pp + ln + 4].tobytes(), "little") == oracle.xxh32(data[pos:pos + ln]), pos
        pos += ln
    assert pos == n and np.array_equal(f[wb[7][0]:wb[7][0] + 65536], data[7 << 16:8 << 16])
    COVER["many"].add("write")


def test_coverage_reached():
    """What the sweeps above (run first) reached, the way tests/test_gpu_grammar.py's test_path_bits_seen holds its file to its claim."""
    missing = [(f, s) for f in ac.FINDERS for s in range(16) if (f, s) not in COVER["enc"]]
    assert not missing, ("finder x source residue", missing)
    missing = [(e, d) for e in range(len(ENVS)) for d in range(16) if (e, d) not in COVER["env_dst"]]
    assert not missing, ("switch set x destination residue", missing)
    for entry in ("frame", "blocks", "blocks_indexed", "inband", "frames"):
        assert {f for e, f, _ in COVER["dec"] if e == entry} == set(range(16)), ("frame residues", entry)
        assert {d for e, _, d in COVER["dec"] if e == entry} == set(range(16)), ("destination residues", entry)
    for what in ("xxh_blocks", "xxh_write_blocks"):
        short = {n: sorted(COVER[what][n]) for n in ac.XXH_LENS if n and len(COVER[what][n]) < 4}
        assert not short, (what, short)
    for what in ("xxh_content", "xxh_write_content"):
        short = {n: sorted(COVER[what][n]) for n in ac.XXH_LENS if len(COVER[what][n]) < 4}
        assert not short, (what, short)
    assert COVER["many"] == {"verify", "write"}
