"""The index model (tests/lz4_index.py) against the independent ground truth of tests/lz4_grammar.py: the sequences each grammar
frame was written with.  No GPU: what the decoders are then held to (tests/test_gpu_index_forgery.py) is only as good as this."""
import hashlib

import numpy as np
import pytest

import lz4_grammar as G
import lz4_index as X

LAST = "carrier/indep6/sparse/k5"          # the corpus is generated in order; the dense carriers behind this one cost seconds each


@pytest.fixture(scope="module")
def frames():
    out = []
    for name, fr in G._frames():
        b = fr.bytes()
        try:
            P = X.Parsed(b)
        except ValueError:
            out.append((name, b, None, fr.planted))      # cut payloads (lit/cut/*): not a frame an index can describe
        else:
            out.append((name, b, P, fr.planted))
        if name == LAST: break
    return out


def _forgery_frame():
    """Three 256 KiB blocks (four chunks each) of sparse sequences, a stored block, and a short last block."""
    fr = G.Frame(5, rng=G._rng("index-forgery-frame"))
    for _ in range(3):
        b = fr.block(); b.sparse(fr.bs - 12); b.end(12)
    fr.stored(fr.rng.integers(0, 256, fr.bs, dtype=np.uint8).tobytes())
    b = fr.block(); b.sparse(70000); b.end(9)
    return fr.bytes()


def test_parse_and_build_follow_the_planted_sequences(frames):
    """The parser finds exactly the sequences lz4_grammar wrote, and build() puts an entry at every 16th sequence of a chunk (the
    chunk of the match's start), the first of each block at sequence 0, with the planted in_off / out_pos."""
    blocks_seen = chunked = 0
    for name, b, P, planted in frames:
        if P is None: continue
        assert len(P.blocks) == len(planted), name
        ix = X.build(b, P)
        V = X.View(ix)
        chunk = X.pick_chunk_size(P.bs)
        for k, (B, want) in enumerate(zip(P.blocks, planted)):
            if want is None: continue
            assert not B["stored"], (name, k)
            want = np.array(want, dtype=np.int64).reshape(-1, 5)
            assert np.array_equal(B["seqs"], want), (name, k)
            blocks_seen += 1
            # the planted list alone says where the entries go
            ms = want[:-1, 1] + want[:-1, 2]
            cid = ms // chunk
            starts = [0] if len(want) == 1 else [i for i in range(len(want) - 1) if i == 0 or cid[i] != cid[i - 1] or
                                                  (i - np.searchsorted(cid, cid[i])) % X.IX_STRIDE == 0]
            e = V.entries[int(V.blocks[k, 2]):int(V.blocks[k, 2]) + int(V.blocks[k, 3])]
            assert [int(x) for x in e[:, 2]] == starts, (name, k)
            assert np.array_equal(e[:, 0], want[starts, 0]) and np.array_equal(e[:, 1], want[starts, 1]), (name, k)
            assert [int(x) >> 8 for x in e[:, 3]] == [k] * len(e), (name, k)
            assert int((e[:, 3] & 0xFF).sum()) == len(want), (name, k)
            chunked += len(set(cid.tolist())) > 1
    assert blocks_seen > 500 and chunked >= 4, (blocks_seen, chunked)


def test_build_is_truthful_for_every_frame(frames):
    """Every frame that parses - grammar frames of every family and framing, liblz4's own frames - gets a truthful index and a
    truthful trailer from the model."""
    import oracle
    from lz4_frame_conduit_amd import datagen
    n = 0
    for name, b, P, _ in frames:
        if P is None: continue
        ix = X.build(b, P)
        assert X.violations(b, ix, P) == [], name
        assert X.trailer_violations(b + X.trailer(b, ix, P), len(b)) == [], name
        assert X.trailer_violations(b + X.trailer(b, None, P), len(b)) == [], name
        n += 1
    data = datagen.synth50(3 << 20, 8).tobytes()
    for kw in (dict(bsid=4, indep=1), dict(bsid=5, indep=0, bck=1), dict(bsid=7, indep=1, cck=1)):
        b = oracle.conduit_compress(data, oracle.mkprefs(**kw))            # == liblz4's frame
        P = X.Parsed(b)
        assert P.content == len(data)
        ix = X.build(b, P)
        assert X.violations(b, ix, P) == [], kw
        n += 1
    assert n > 500


def test_every_forgery_is_caught_by_the_model():
    """Each named forgery breaks one thing: the model refuses every one, in the index and spliced into the trailer."""
    b = _forgery_frame()
    P = X.Parsed(b)
    ix = X.build(b, P)
    assert X.truthful(b, ix, P)
    buf = np.concatenate([ix, np.zeros(64 * X.ENT_W, np.uint32)])          # an index buffer with room to spare, as the compressor's
    names = X.forgery_names(b, P)
    assert len(names) == len(set(names)) >= 40 and "table/stored_claims_seqs" in names
    for nm, f in X.forgeries(b, buf, P):
        assert len(f) == len(buf) and not np.array_equal(f, buf), nm
        assert X.violations(b, f, P), nm
    for nm in names:
        s = X.forge_trailer(b, buf if nm.startswith("header/total_entries") else ix, nm, P)
        assert X.trailer_violations(s, len(b)), nm


def test_block_table_forgeries_break_one_link_only():
    """The suffix shifts keep every link but the one in front of block k (the gap k_copy_selffed's per-workgroup checks left
    open): the model shows which links hold.  (Links in 32-bit arithmetic: D = 2^32 - base - 1 keeps them only modulo 2^32, which a
    decoder summing in 32 bits would miss at block k's own end as well.)"""
    b = _forgery_frame()
    P = X.Parsed(b)
    ix = X.build(b, P)
    for D in ("1", "64", "2^20", "0x7FFFFFFF", "2^32-base-1"):
        f = X.forge(b, ix, "table/seq_suffix_shift/" + D, P)
        bl = X.View(f).blocks.astype(np.int64)
        ends = (bl[:, 0] + bl[:, 1]) & 0xFFFFFFFF
        broken = [i for i in range(len(bl) - 1) if ends[i] != bl[i + 1, 0]]
        assert len(broken) == 1 and int(X.View(f).blocks[broken[0] + 1, 0]) != int(X.View(ix).blocks[broken[0] + 1, 0]), (D, broken)


def test_forgery_list_is_stable():
    """Rebuilt from the names alone: the same bytes on every run."""
    def digest():
        b = _forgery_frame()
        P = X.Parsed(b)
        ix = X.build(b, P)
        h = hashlib.sha256(X.index_bytes(ix))
        for nm in X.forgery_names(b, P):
            h.update(nm.encode())
            h.update(X.forge_trailer(b, ix, nm, P)[len(b):])
        return h.hexdigest()
    assert digest() == digest()
