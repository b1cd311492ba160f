"""Every decode path that consumes a sequence index, against indexes that lie consistently (tests/lz4_index.py forgeries), and the
compressor's own index held to the model.  The promise under test (include/lz4f_mi355x.h, "Sequence index"): a stale, foreign or
lying index may cost time, never change the output, and never make a kernel write outside the caller's buffer."""
import numpy as np
import pytest

import lz4_grammar as G
import lz4_index as X
import oracle
from lz4_frame_conduit_amd import datagen
from test_gpu_parity import PATH, prefs_of

pytestmark = pytest.mark.gpu

SWITCHES = {"default": {}, "no_selffeed": {"LZ4F_MI355X_NO_SELFFEED": "1"}, "trace_always": {"LZ4F_MI355X_TRACE_ALWAYS": "1"},
            "trace_hops": {"LZ4F_MI355X_TRACE_ALWAYS": "1", "LZ4F_MI355X_NO_DOUBLING": "1"}}
GUARD = 4096
REACHED = set()                                            # index-consuming path bits seen by the tests of this module


def _engine(monkeypatch, env):
    from lz4_frame_conduit_amd.device import Engine
    for k in ("LZ4F_MI355X_NO_SELFFEED", "LZ4F_MI355X_TRACE_ALWAYS", "LZ4F_MI355X_NO_DOUBLING"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Engine(0)                                      # (switches are read when an engine is made)


def _dev(b: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def _out(n):
    """An output buffer of n bytes with a guard pattern behind it: (whole, the view handed to the decoder)."""
    import torch
    whole = torch.zeros(n + GUARD, dtype=torch.uint8, device="cuda")
    whole[n:] = torch.arange(GUARD, dtype=torch.int32, device="cuda").remainder(251).to(torch.uint8) + 1
    return whole, whole[:n]


def _guard_intact(whole, n):
    import torch
    want = torch.arange(GUARD, dtype=torch.int32, device="cuda").remainder(251).to(torch.uint8) + 1
    return torch.equal(whole[n:], want)


def _note(flags):
    p = int(flags) >> 12
    for k in ("indexed", "doubling", "hops", "dropped"):
        if p & PATH[k]: REACHED.add(k)
    return p


def _refused(path):
    """The index given was not what decoded: no indexed kernels, or they gave up (DROPPED), or the host set the index aside
    before any kernel saw it and the decoder indexed the frame itself (SELF_INDEX: a linked frame whose header is not this
    library's, engine.hip launch_decompress)."""
    return not path & PATH["indexed"] or path & PATH["dropped"] or path & PATH["self_index"]


def _inputs():
    rng = np.random.default_rng(71)
    yield "synth50", datagen.synth50(4 << 20, 71)
    yield "structured", np.frombuffer(datagen.structured((3 << 20) + 555, 72), dtype=np.uint8).copy()
    yield "text", datagen.synth_text(2 << 20, 73)
    yield "stored-mixed", np.concatenate([datagen.synth50(2 << 20, 74), rng.integers(0, 256, 1 << 20, dtype=np.uint8), datagen.synth50(1 << 20, 75)])
    yield "zeros", np.zeros(2 << 20, dtype=np.uint8)


FRAMINGS = [(4, 1, 0), (5, 1, 1), (6, 1, 0), (7, 1, 1), (4, 0, 0), (5, 0, 1), (6, 0, 0), (7, 0, 1)]     # bsid, independent, block checksums


def _takes_index(bsid, indep):
    # engine.hip launch_decompress: the indexed kernels are the 'f' mode's - linked frames and blocks of 256 KiB and more;
    # independent 64 KiB blocks go to the wave-per-block decoder ('1'), which has no use for an index
    return not indep or bsid >= 5


@pytest.mark.parametrize("det", [False, True])
def test_compressor_index_is_true_and_used(monkeypatch, det):
    """The compressor's index and trailer agree with the model in every field, the footer's counts with the header's, and the
    decoder uses every usable index it is given (PATH_INDEXED, never PATH_INDEX_DROPPED)."""
    import torch
    eng = _engine(monkeypatch, {})
    eng.set_deterministic(det)
    usable = 0
    for name, data in _inputs():
        src = torch.from_numpy(data).cuda()
        n = src.numel()
        for bsid, indep, bck in FRAMINGS:
            kw = dict(bsid=bsid, indep=indep, bck=bck)
            p = prefs_of(kw)
            bs = 1 << (8 + 2 * bsid)
            nb = (n + bs - 1) // bs
            # explicit index
            frame = torch.empty(eng.frame_bound(n, p), dtype=torch.uint8, device="cuda")
            table, index = eng.new_table(nb), eng.new_index(n, p)
            eng.compress_async(src, frame, p, table, index)
            r = eng.result()
            fb = frame[:r.size].cpu().numpy().tobytes()
            ix = index.cpu().numpy().view(np.uint32)
            P = X.Parsed(fb)
            ok = X.usable_by_decoder(ix)
            if ok:
                usable += 1
                assert X.violations(fb, ix, P) == [], (name, kw, det, X.violations(fb, ix, P)[:4])
            whole, back = _out(n)
            eng.decompress_blocks_async(frame, r.size, back, table, nb, p.frameInfo, index)
            r2 = eng.result()
            assert r2.size == n and torch.equal(back, src) and _guard_intact(whole, n), (name, kw, det)
            path = _note(r2.flags)
            if ok and _takes_index(bsid, indep):
                assert path & PATH["indexed"] and not path & PATH["dropped"], (name, kw, det, hex(path))
            # in-band trailer
            frame2 = torch.empty(eng.frame_bound_inband(n, p), dtype=torch.uint8, device="cuda")
            eng.compress_async(src, frame2, p, inband=True)
            r3 = eng.result()
            stream = frame2[:r3.size].cpu().numpy().tobytes()
            P2 = X.Parsed(stream)
            assert X.trailer_violations(stream, P2.end) == [], (name, kw, det, X.trailer_violations(stream, P2.end)[:4])
            lst, tix, ft = X.read_trailer(stream, P2.end)
            if tix is not None:
                assert (ft["total_seqs"], ft["total_entries"]) == (int(tix[3]), int(tix[4])), (name, kw, det)
                assert X.violations(stream[:P2.end], tix, P2) == [], (name, kw, det)
            whole, back = _out(n)
            eng.decompress_frame_async(frame2, int(r3.size), back)
            r4 = eng.result()
            assert r4.size == n and torch.equal(back, src) and _guard_intact(whole, n), (name, kw, det)
            path = _note(r4.flags)
            if tix is not None and _takes_index(bsid, indep):
                assert path & PATH["indexed"] and not path & PATH["dropped"], (name, kw, det, hex(path))
    assert usable >= 25, usable
    eng.close()


def _forgery_cases():
    """(name, data, prefs kw): independent 1 MiB blocks with a stored block inside (k_copy_selffed / k_parse_indexed + k_copy_indexed /
    the tracers), and linked 64 KiB blocks (k_copy_indexed's linked groups)."""
    rng = np.random.default_rng(81)
    yield "indep1m", np.concatenate([datagen.synth50(2 << 20, 81), rng.integers(0, 256, 1 << 20, dtype=np.uint8), datagen.synth50(3 << 20, 82)[:(2 << 20) + 4321]]), dict(bsid=6, indep=1)
    yield "linked64k", datagen.synth50(2 << 20, 83)[:(1 << 20) + 999].copy(), dict(bsid=4, indep=0)


@pytest.mark.parametrize("sw", list(SWITCHES))
def test_forged_indexes_never_change_the_output(monkeypatch, sw):
    """Every forgery of tests/lz4_index.py through both entry points that take an index - decompress_blocks_async with the
    forged index, decompress_frame_async with it spliced into the trailer - under each set of switches: the input comes back,
    nothing is written behind the capacity, and a forged block table or header is refused (_refused)."""
    import torch
    eng = _engine(monkeypatch, SWITCHES[sw])
    for cname, data, kw in _forgery_cases():
        src = torch.from_numpy(data).cuda()
        n = src.numel()
        p = prefs_of(kw)
        bs = 1 << (8 + 2 * kw["bsid"])
        nb = (n + bs - 1) // bs
        frame = torch.empty(eng.frame_bound(n, p), dtype=torch.uint8, device="cuda")
        table, index = eng.new_table(nb), eng.new_index(n, p)
        eng.compress_async(src, frame, p, table, index)
        r = eng.result()
        fb = frame[:r.size].cpu().numpy().tobytes()
        P = X.Parsed(fb)
        buf = index.cpu().numpy().view(np.uint32).copy()
        assert X.truthful(fb, buf, P), cname
        true_ix = buf[:X.fixed_words(int(buf[1]), int(buf[2])) + int(buf[4]) * X.ENT_W]
        model = X.build(fb, P)

        def run_blocks(ix_words):
            whole, back = _out(n)
            eng.decompress_blocks_async(frame, r.size, back, table, nb, p.frameInfo, _dev(X.index_bytes(ix_words)))
            rr = eng.result()
            assert _guard_intact(whole, n)
            return rr, back

        def run_stream(stream):
            whole, back = _out(n)
            eng.decompress_frame_async(_dev(stream), len(stream), back)
            rr = eng.result()
            assert _guard_intact(whole, n)
            return rr, back

        # controls: the true index and the model's are taken
        for label, ixw in (("compressor", buf), ("model", model)):
            rr, back = run_blocks(ixw)
            path = _note(rr.flags)
            assert rr.size == n and torch.equal(back, src), (cname, sw, label)
            assert path & PATH["indexed"] and not path & PATH["dropped"], (cname, sw, label, hex(path))
        rr, back = run_stream(fb + X.trailer(fb, model, P))
        path = _note(rr.flags)
        assert rr.size == n and torch.equal(back, src) and path & PATH["trailer"], (cname, sw)
        assert path & PATH["indexed"] and not path & PATH["dropped"], (cname, sw, "model trailer", hex(path))
        for nm in X.forgery_names(fb, P):
            refused_expected = nm.startswith("table/") or nm.startswith("header/")
            if not nm.startswith("footer/"):
                rr, back = run_blocks(X.forge(fb, buf, nm, P))
                path = _note(rr.flags)
                assert rr.size == n and torch.equal(back, src), (cname, sw, nm, "blocks")
                if refused_expected:
                    assert _refused(path), (cname, sw, nm, "blocks", hex(path))
            base = buf if nm.startswith("header/total_entries") else true_ix
            rr, back = run_stream(X.forge_trailer(fb, base, nm, P))
            path = _note(rr.flags)
            assert rr.size == n and torch.equal(back, src), (cname, sw, nm, "trailer")
            if refused_expected:
                assert _refused(path), (cname, sw, nm, "trailer", hex(path))
    eng.close()


def _linked_frame(short_mid: bool):
    """64 KiB linked blocks of sparse sequences; short_mid: the second and fourth are short, as liblz4 writes them on a flush."""
    fr = G.Frame(4, linked=True, rng=G._rng("linked-short-%d" % short_mid))
    for size in ((fr.bs, 1000, fr.bs, 5000, fr.bs, 30000) if short_mid else (fr.bs,) * 5 + (30000,)):
        b = fr.block(); b.sparse(size - 12); b.end(12)
    return fr.bytes(), bytes(fr.out)


def _grammar_short_mid():
    out = []
    for name, fr in G._frames():                          # (in corpus order: stop before the carriers)
        if name.startswith("blk/linked/short_mid/"): out.append((name, fr.bytes(), len(fr.out)))
        if name.startswith("carrier/"): break
    return out


def test_linked_frame_with_short_inner_blocks_through_the_trailer(monkeypatch):
    """A valid linked frame with flushed (short) inner blocks and a true trailer index: liblz4's bytes.  The indexed decode
    assumes every block but the last is full; it must notice that it is not and hand the frame to the generic linked decoder.
    The control - same geometry, full blocks - takes the indexed path, so the model's trailers are accepted when true."""
    import torch
    for sw in ("default", "trace_always"):
        eng = _engine(monkeypatch, SWITCHES[sw])
        for short_mid in (False, True):
            fb, content = _linked_frame(short_mid)
            ref, used = oracle.decompress_frame(fb, cap=len(content) + 64)
            assert used == len(fb) and ref == content
            P = X.Parsed(fb)
            stream = fb + X.trailer(fb, X.build(fb, P), P)
            cap = len(P.blocks) * P.bs                     # (the device decoders' room: every block full - as tests/test_gpu_grammar.py gives them)
            whole, back = _out(cap)
            eng.decompress_frame_async(_dev(stream), len(stream), back)
            rr = eng.result()
            path = _note(rr.flags)
            assert _guard_intact(whole, cap)
            assert rr.size == len(content) and back[:rr.size].cpu().numpy().tobytes() == content, (sw, short_mid, hex(path))
            if not short_mid:
                assert path & PATH["trailer"] and path & PATH["indexed"] and not path & PATH["dropped"], (sw, hex(path))
        for name, fr_b, content in (_grammar_short_mid() if sw == "default" else []):
            ref, used = oracle.decompress_frame(fr_b, cap=content + 64)
            P = X.Parsed(fr_b)
            stream = fr_b + X.trailer(fr_b, X.build(fr_b, P), P)
            cap = len(P.blocks) * P.bs
            whole, back = _out(cap)
            eng.decompress_frame_async(_dev(stream), len(stream), back)
            rr = eng.result()
            _note(rr.flags)
            assert _guard_intact(whole, cap)
            assert used == len(fr_b) and rr.size == len(ref) == content and back[:rr.size].cpu().numpy().tobytes() == ref, name
        eng.close()


def test_every_index_path_was_reached():
    """The tests above went through every index-consuming path: the indexed kernels, the pointer doubling, the hop-by-hop
    tracer, and the drop to the generic decoder."""
    assert REACHED >= {"indexed", "doubling", "hops", "dropped"}, REACHED
