"""Every decoder's match copies on planted dependency patterns (tests/match_dep_cases.py), byte for byte against the sequential
model.  One test per route; each sends every case of the framings the route takes.

Per call: the output buffer is pre-filled with the COMPLEMENT of the expected bytes (a match copied before its source was
written reads a byte that is wrong at every position), a guard behind the capacity must stay intact, and size and bytes must
equal the model's - no tolerance, no exempt case.  A failure names the case, the route, the switch set, the first differing
output position and the sequence that owns it.

Routes:
  1. lz4f_mi355x_decompressFrame (host pointers; test_gpu_grammar.host_call keeps its own 0xA5 fill and compares a hash, so the
     complement-filled call is made here and host_call is run beside it) and LZ4F_decompress whole (stream_call).
  2. Engine.decompress_frame_async under each switch set of test_gpu_grammar.ENVS.
  3. Engine.decompress_blocks_async with the frame's table and the honest index of lz4_index.build, for the framings that take
     an index (engine.hip dec_index: mode 'f' - everything but independent 64 KiB blocks).  Switch sets (Switches::read and
     ix_route / dec_indexed / decode_plan, which is where each is used):
       default              independent: k_copy_selffed; linked: k_parse_indexed + k_resolve_direct + k_copy_indexed in groups
       NO_SELFFEED          independent blocks through k_parse_indexed + k_resolve_direct + k_copy_indexed too
       TRACE_ALWAYS         gate 2: k_build_postab + k_pd_init + 12 x k_pd_round decode every frame
       TRACE_ALWAYS+NO_DOUBLING   ... k_trace_copy instead
       NO_RESOLVE           k_copy_indexed with no resolved sources: every match that the parse did not mark stays on the chain
                            (longer dependency chains through fz_copier's replay and a fuller set-aside list)
       NO_GROUPS            linked: one block per workgroup - every block's reads in front of it are another workgroup's (set aside)
       GROUP_KIB=128        linked 64 KiB: groups of two - the list carried and rebased inside a group, at other blocks than by default
       FEED_ROUND=24        k_copy_selffed parses in rounds of 24 sequences: its position ring turns over at other sequences
       CHAIN_GATE=4         linked frames with over a quarter of their sequences on the chain are handed to k_decode_linked
                            BY the indexed kernels (IX_CHAIN_GATED): the drop itself is on purpose and shows as `dropped`
     NO_TRACE is left out: without TRACE_ALWAYS the corpus' frames are not dense by the gate, so it changes no copy code here.
  4. The same frames with the in-band trailer (lz4_index.trailer + splice) through decompress_frame_async, default switches and
     TRACE_ALWAYS.
  5. decompress_frames_async, one batch per framing with all its cases (k_bf_blocks, k_bf_serial).
Dictionaries are out of scope (dict_cases.py pins that seam).

Path bits (result.flags >> 12): every call's bits are compared EXACTLY with what decode_plan, dec_index, ix_route, dec_indexed
and dec_generic give for that case under that switch set (_expect_frame, _expect_indexed, _tracer_bits; walk_delivered, which
names no decoder, is left out):
  route 2   i64: wave_per_block alone.  Others: fused (launched behind whatever ran), window for linked frames unless NO_WINDOW;
            where a self-index is made (linked frames; independent blocks that k_density_probe - modelled by
            Analysis.probe_dense - does not call dense and that have no run beyond SPX_LANE_HOPS, unless NO_SPX / NO_SELFINDEX) self_index, indexed and the tracer the index's density and the switches select; otherwise, for
            independent blocks, wave_per_block and (unless DENSE_MODE=2) workgroup_per_block
  route 3   table, indexed, fused, window (linked), and doubling or hops as ix_route selects them
  route 4   trailer instead of table, otherwise as route 3
  route 5   batch
  dropped   nowhere - except, by design: CHAIN_GATE (above), the deep/ cases the hop tracer may hand on (Case.may_drop: chains
            beyond IXT_MAX_HOPS hops when a region in front is not complete yet; the other bits stay as stated), and frames dense
            by their sequence count where the block table holds capacities (route 3's second table, route 4 with room to spare)
What the bits cannot say: doubling and hops are set when the host launches a tracer.  A tracer that refuses on the device
(ixt_fail) leaves the frame to the copier workgroups without a flag, so these bits do not prove that a tracer produced a
case's bytes; only the sensitivity builds (g) and (h) of DESIGN.md section 5 show that they do for the cases named there.
The last test asserts that every bit aimed at was seen, per family (AIMS).

Measured on the MI355X (337 cases): route 1 1011 calls in 0.7 s; route 2 337 calls in 0.15-0.29 s per switch set; route 3 288
calls in 0.09-0.19 s per switch set (default: 576 in 0.25 s); route 4 576 in 0.25 s (default) and 288 in 0.09 s; route 5 six batches in 0.04 s; the module
23 s, 16 of them building the corpus on the host.  DESIGN.md section 5 has the sensitivity table."""
import ctypes
import hashlib
import os
import time

import numpy as np
import pytest

import lz4_index as X
import match_dep_cases as M
from lz4_frame_conduit_amd import _ffi
from test_gpu_grammar import DROPPED, ENVS, L, PATH, host_call, stream_call       # noqa: F401  (L: a fixture)
from test_gpu_index_forgery import GUARD, _guard_intact, _out

pytestmark = pytest.mark.gpu
sha = lambda b: hashlib.sha256(b).hexdigest()
BITS = dict(PATH, trailer=0x002, dropped=DROPPED, batch=0x1000)
TAKES_INDEX = ("i256", "i4m", "l64", "l256", "l4m")
IX_ENVS = [("default", {}), ("no_selffeed", {"LZ4F_MI355X_NO_SELFFEED": "1"}), ("trace_always", {"LZ4F_MI355X_TRACE_ALWAYS": "1"}),
           ("trace_hops", {"LZ4F_MI355X_TRACE_ALWAYS": "1", "LZ4F_MI355X_NO_DOUBLING": "1"}), ("no_resolve", {"LZ4F_MI355X_NO_RESOLVE": "1"}),
           ("no_groups", {"LZ4F_MI355X_NO_GROUPS": "1"}), ("group_kib128", {"LZ4F_MI355X_GROUP_KIB": "128"}),
           ("feed_round24", {"LZ4F_MI355X_FEED_ROUND": "24"}), ("chain_gate4", {"LZ4F_MI355X_CHAIN_GATE": "4"})]
# which decoders each family is for, as the path bits name them
AIMS = dict(period={"wave_per_block", "fused", "window", "indexed", "self_index", "batch"}, slot={"fused", "indexed", "self_index"},
            window={"wave_per_block", "workgroup_per_block", "batch"}, direct={"indexed", "self_index", "doubling", "hops"},
            link={"indexed", "window", "self_index", "batch"}, deep={"doubling", "hops", "indexed", "workgroup_per_block"},
            ring={"window", "workgroup_per_block", "indexed", "batch"})
GAP = 64                         # route 5: guard bytes behind every frame of a batch
SEEN = {}                        # family -> names of the path bits seen
ROUTES_RUN = set()


class Dev:
    """The corpus on the device, made once: per case the frame, the expected bytes and their complement."""

    def __init__(self):
        import torch
        self.items = []
        for c, fb, out in M.corpus():
            exp = torch.from_numpy(np.frombuffer(out, dtype=np.uint8).copy()).cuda()
            fr = torch.from_numpy(np.frombuffer(fb + bytes(32), dtype=np.uint8).copy()).cuda()
            P = X.Parsed(fb)
            seqs = sum(len(B["seqs"]) for B in P.blocks if not B["stored"])
            self.items.append(dict(c=c, fb=fb, out=out, exp=exp, fill=torch.bitwise_not(exp), fr=fr, nblk=len(P.blocks), seqs=seqs,
                                   dense=not P.linked and P.bsid >= 5 and M.Analysis(fb).probe_dense()))


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _engine(monkeypatch, env):
    from lz4_frame_conduit_amd.device import Engine
    for k in {k for e in ENVS + [e for _, e in IX_ENVS] for k in e}: monkeypatch.delenv(k, raising=False)
    for k, v in env.items(): monkeypatch.setenv(k, v)
    return Engine(0)                                      # (switches are read when an engine is made)


def _buffer(it, cap):
    whole, back = _out(cap)
    n = len(it["out"])
    back[:n] = it["fill"]
    if cap > n: back[n:] = 0x5A
    return whole, back


def _note(c, flags):
    p = int(flags) >> 12
    SEEN.setdefault(c.family, set()).update(k for k, v in BITS.items() if p & v)
    return p


def _explain(it, got: bytes):
    """Where the first wrong byte is and whose it is."""
    exp = it["out"]
    n = min(len(got), len(exp))
    a, b = np.frombuffer(got[:n], dtype=np.uint8), np.frombuffer(exp[:n], dtype=np.uint8)
    d = np.flatnonzero(a != b)
    if len(d) == 0: return "sizes differ: %d, expected %d" % (len(got), len(exp))
    pos = int(d[0])
    A = M.Analysis(it["fb"])
    blk, i, kind = M.owner(A, pos)
    what = ""
    if i is not None:
        at, op, lit, ml, off = (int(x) for x in A.S(blk)[i])
        what = " = block %d sequence %d (output %d: %d literals, match of %d from %d back), its %s byte %d" % (
            blk, i, op, lit, ml, off, kind, pos - A.P.blocks[blk]["out_off"] - (op if kind == "literal" else op + lit))
    return "%d of %d bytes differ, the first at output position %d%s: got %#04x (fill %#04x), expected %#04x; aim: %s" % (
        len(d), n, pos, what, int(a[pos]), int(b[pos]) ^ 0xFF, int(b[pos]), it["c"].aim)


def _has(env, k): return "LZ4F_MI355X_" + k in env


def _tracer_bits(linked, bs, env, n_ix, seqs):
    """engine.hip ix_route + dec_indexed: which tracer the host sets up behind an index of `seqs` sequences laid out for n_ix blocks."""
    ta, nr = _has(env, "TRACE_ALWAYS"), _has(env, "NO_RESOLVE")
    doubling = (seqs * 48 > n_ix * bs or ta) and not _has(env, "NO_DOUBLING")
    selffed = not linked and not _has(env, "NO_SELFFEED") and not nr and not ta and not doubling
    trace_can = not _has(env, "NO_TRACE") and not nr
    gate = 0 if not trace_can else 2 if ta else 1 if (linked or doubling) else 0
    if selffed or not gate: return set()                   # (k_copy_selffed is one kernel; no gate: the copier workgroups alone)
    return {"doubling"} if doubling else {"hops"}


def _expect_indexed(it, env, how):
    """Routes 3 and 4: the index comes with the call (`how`: table or trailer) and is laid out for the frame's own block count; the
    generic kernels are launched behind (fused; window for a linked frame) and return at once."""
    c = it["c"]
    # (window: decode_plan leaves a linked frame of ONE block with a caller's table to the fused workgroup)
    windowed = c.fr.linked and not (how == "table" and it["nblk"] == 1)
    return {how, "indexed", "fused"} | ({"window"} if windowed else set()) | _tracer_bits(c.fr.linked, c.fr.bs, env, it["nblk"], it["seqs"])


def _expect_frame(it, env, cap):
    """Route 2, decode_plan and the stages behind it for a frame without an index.  The two device verdicts that are read back or
    visible are predicted from the case: k_density_probe's by the model of it (Analysis.probe_dense; the CPU test holds Case.dense
    to it), the stretch self-index's success from the frame being valid and having no run beyond SPX_LANE_HOPS (Case.spx_long)."""
    c = it["c"]
    if c.framing == "i64": return {"wave_per_block"}
    linked, bs = c.fr.linked, c.fr.bs
    bits = {"fused"} | ({"window"} if linked and not _has(env, "NO_WINDOW") else set())
    tries = not _has(env, "NO_SELFINDEX") and (linked or not _has(env, "NO_SPX"))
    if tries and (linked or not (it["dense"] or c.spx_long)):      # (a dense payload of independent blocks, a stretch too long: the walk declines)
        n_max = min(cap // bs + 2, len(it["fb"]) // 5 + 2)     # (dev_decompressFrame: the index is laid out for the call's upper bound)
        return bits | {"self_index", "indexed"} | _tracer_bits(linked, bs, env, n_max, it["seqs"])
    if not linked: bits |= {"wave_per_block"} | (set() if env.get("LZ4F_MI355X_DENSE_MODE") == "2" else {"workgroup_per_block"})
    return bits


IGNORED = DROPPED | 0x2000       # dropped: judged apart; walk_delivered names no decoder (tests/test_gpu_walks.py pins it)


def _check(bad, it, route, sw, r, err, whole, back, cap, expect, drop_ok=False):
    import torch
    c = it["c"]
    n = len(it["out"])
    if not _guard_intact(whole, cap): bad.append((c.name, route, sw, "bytes behind the capacity were written"))
    if err is not None: bad.append((c.name, route, sw, "error: " + err)); return
    p = _note(c, r.flags)
    if r.size != n or not torch.equal(back[:n], it["exp"]):
        bad.append((c.name, route, sw, "path %#x size %d: " % (p, r.size) + _explain(it, back[:min(int(r.size), n)].cpu().numpy().tobytes())))
    want = 0
    for k in expect: want |= BITS[k]
    if (p & ~IGNORED) != want:
        name = lambda v: " ".join(sorted(k for k, b in BITS.items() if v & b)) or "-"
        bad.append((c.name, route, sw, "path %#x: expected exactly [%s], lacks [%s], shows [%s]" % (p, name(want), name(want & ~p), name(p & ~IGNORED & ~want))))
    if p & DROPPED and not drop_ok: bad.append((c.name, route, sw, "path %#x shows dropped" % p))


def _report(route, sw, calls, t0, bad):
    print("match deps, %s under %s: %d calls in %.2f s" % (route, sw or "default", calls, time.time() - t0))
    for b in bad[:40]: print("   ", *b)
    assert not bad, (len(bad), bad[:6])


def test_route1_host_pointers_and_stream(L, dev):
    t0, bad, calls = time.time(), [], 0
    L.lz4f_mi355x_release_engines()
    for it in dev.items:
        c, fb, out = it["c"], it["fb"], it["out"]
        n = len(out)
        fill = bytes(np.bitwise_not(np.frombuffer(out, dtype=np.uint8)))
        buf = ctypes.create_string_buffer(fill + b"\xa5" * GUARD, n + GUARD)
        used = ctypes.c_size_t(0)
        r = L.lz4f_mi355x_decompressFrame(buf, n, fb, len(fb), ctypes.byref(used))
        calls += 1
        if buf.raw[n:] != b"\xa5" * GUARD: bad.append((c.name, "host", "", "bytes behind the capacity were written"))
        if L.LZ4F_isError(r): bad.append((c.name, "host", "", L.LZ4F_getErrorName(r).decode()))
        elif r != n or buf.raw[:n] != out: bad.append((c.name, "host", "", _explain(it, buf.raw[:min(r, n)])))
        elif used.value != len(fb): bad.append((c.name, "host", "", "consumed %d of %d" % (used.value, len(fb))))
        err, got = host_call(L, fb, n + 5)
        calls += 1
        if err or got != sha(out): bad.append((c.name, "host@+5", "", err or "other bytes"))
        err, got = stream_call(L, fb)
        calls += 1
        if err or got != sha(out): bad.append((c.name, "stream", "", err or "other bytes"))
    ROUTES_RUN.add(1)
    _report("host pointers + LZ4F_decompress", "", calls, t0, bad)


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=["+".join(k[len("LZ4F_MI355X_"):] + ("=" + v if v != "1" else "") for k, v in e.items()) or "default" for e in ENVS])
def test_route2_frame_async(monkeypatch, dev, ei):
    from lz4_frame_conduit_amd.device import DeviceCodecError
    env = ENVS[ei]
    sw = " ".join("%s=%s" % (k[len("LZ4F_MI355X_"):], v) for k, v in env.items())
    eng = _engine(monkeypatch, env)
    t0, bad, calls = time.time(), [], 0
    for it in dev.items:
        c = it["c"]
        cap = len(it["out"])
        whole, back = _buffer(it, cap)
        try:
            eng.decompress_frame_async(it["fr"], len(it["fb"]), back); r = eng.result(); err = None
        except DeviceCodecError as e:
            r, err = None, str(e)
        calls += 1
        _check(bad, it, "frame_async", sw, r, err, whole, back, cap, _expect_frame(it, env, cap), _drop_allowed(c, env))
    eng.close()
    ROUTES_RUN.add((2, ei))
    _report("decompress_frame_async", sw, calls, t0, bad)


def _table(it):
    import torch
    P = X.Parsed(it["fb"])
    ent = np.zeros(len(P.blocks) + 1, dtype=np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("word", "<u4"), ("dst_size", "<u4")]))
    for i, B in enumerate(P.blocks):
        ent[i] = (B["src_off"], i * P.bs, B["csize"] | (0x80000000 if B["stored"] else 0), B["out_len"])      # as the compressor leaves it: decoded sizes
    room = ent.copy()
    room["dst_size"][:len(P.blocks)] = P.bs                 # as the header describes a caller's table: every block's capacity
    info = _ffi.FrameInfo()
    info.blockSizeID, info.blockMode, info.blockChecksumFlag = P.bsid, 0 if P.linked else 1, int(P.bck)
    ix = X.build(it["fb"], P)
    dv = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    nseq = sum(len(B["seqs"]) for B in P.blocks if not B["stored"])
    return dict(P=P, n=len(P.blocks), tb=dv(ent.tobytes()), tb_room=dv(room.tobytes()), dense_by_count=nseq * 20 > P.content, info=info, ix=dv(X.index_bytes(ix)),
                stream=dv(X.splice(it["fb"], X.trailer(it["fb"], ix, P)) + bytes(32)), stream_len=len(it["fb"]) + len(X.trailer(it["fb"], ix, P)))


@pytest.fixture(scope="module")
def tables(dev):
    return {it["c"].name: _table(it) for it in dev.items if it["c"].framing in TAKES_INDEX}


def _drop_allowed(c, env):
    if "LZ4F_MI355X_CHAIN_GATE" in env and c.fr.linked: return True
    return c.may_drop and "LZ4F_MI355X_TRACE_ALWAYS" in env and "LZ4F_MI355X_NO_DOUBLING" in env


@pytest.mark.parametrize("sw", [n for n, _ in IX_ENVS])
def test_route3_blocks_async_with_the_honest_index(monkeypatch, dev, tables, sw):
    from lz4_frame_conduit_amd.device import DeviceCodecError
    env = dict(IX_ENVS)[sw]
    eng = _engine(monkeypatch, env)
    t0, bad, calls = time.time(), [], 0
    for it in dev.items:
        c = it["c"]
        if c.framing not in TAKES_INDEX: continue
        T = tables[c.name]
        cap = T["n"] * T["P"].bs
        whole, back = _buffer(it, cap)
        try:
            eng.decompress_blocks_async(it["fr"], len(it["fb"]), back, T["tb"], T["n"], T["info"], T["ix"]); r = eng.result(); err = None
        except DeviceCodecError as e:
            r, err = None, str(e)
        calls += 1
        _check(bad, it, "blocks_async+index", sw, r, err, whole, back, cap, _expect_indexed(it, env, "table"), _drop_allowed(c, env))
        if sw != "default": continue
        # the same with every block's CAPACITY in the table.  The tracers take a block's size from the table, so with this table they
        # refuse a frame whose last block is short: without notice where the copier workgroups can take over, as `dropped` where the
        # frame is dense by its sequence count alone (over a sequence per 20 bytes: k_resolve_direct was skipped for the tracers' sake)
        whole, back = _buffer(it, cap)
        try:
            eng.decompress_blocks_async(it["fr"], len(it["fb"]), back, T["tb_room"], T["n"], T["info"], T["ix"]); r = eng.result(); err = None
        except DeviceCodecError as e:
            r, err = None, str(e)
        calls += 1
        _check(bad, it, "blocks_async+index, capacity table", sw, r, err, whole, back, cap, _expect_indexed(it, env, "table"), T["dense_by_count"])
    eng.close()
    ROUTES_RUN.add((3, sw))
    _report("decompress_blocks_async with an index", sw, calls, t0, bad)


@pytest.mark.parametrize("sw", ["default", "trace_always"])
def test_route4_in_band_trailer(monkeypatch, dev, tables, sw):
    from lz4_frame_conduit_amd.device import DeviceCodecError
    env = dict(IX_ENVS)[sw]
    eng = _engine(monkeypatch, env)
    t0, bad, calls = time.time(), [], 0
    for it in dev.items:
        c = it["c"]
        if c.framing not in TAKES_INDEX: continue
        T = tables[c.name]
        cap = len(it["out"])
        whole, back = _buffer(it, cap)
        try:
            eng.decompress_frame_async(T["stream"], T["stream_len"], back); r = eng.result(); err = None
        except DeviceCodecError as e:
            r, err = None, str(e)
        calls += 1
        _check(bad, it, "trailer", sw, r, err, whole, back, cap, _expect_indexed(it, env, "trailer"), _drop_allowed(c, env))
        if sw != "default": continue
        # the same with room to spare: the engine's own table then holds a capacity for the last block, not its decoded size (see
        # route 3's capacity table): the tracers may refuse, the bytes and the host's path bits stay
        cap = len(it["out"]) + 4096
        whole, back = _buffer(it, cap)
        try:
            eng.decompress_frame_async(T["stream"], T["stream_len"], back); r = eng.result(); err = None
        except DeviceCodecError as e:
            r, err = None, str(e)
        calls += 1
        _check(bad, it, "trailer, capacity > content", sw, r, err, whole, back, cap, _expect_indexed(it, env, "trailer"), T["dense_by_count"])
    eng.close()
    ROUTES_RUN.add((4, sw))
    _report("decompress_frame_async with the in-band trailer", sw, calls, t0, bad)


def test_route5_batches(monkeypatch, dev):
    import torch
    eng = _engine(monkeypatch, {})
    t0, bad, calls = time.time(), [], 0
    for framing in ("i64", "i256", "i4m", "l64", "l256", "l4m"):
        its = [it for it in dev.items if it["c"].framing == framing]
        so, do = [0], [0]
        for it in its:
            so.append(so[-1] + ((len(it["fb"]) + 32 + 15) & ~15))
            do.append(do[-1] + len(it["out"]) + GAP)        # (a frame's window: its content and a guard of its own behind)
        src = torch.zeros(so[-1], dtype=torch.uint8, device="cuda")
        whole, dst = _out(do[-1])
        for k, it in enumerate(its):
            src[so[k]:so[k] + len(it["fb"])] = it["fr"][:len(it["fb"])]
            dst[do[k]:do[k] + len(it["out"])] = it["fill"]
            dst[do[k] + len(it["out"]):do[k + 1]] = 0xC3
        res = eng.new_results(len(its))
        eng.decompress_frames_async(src, torch.tensor(so, dtype=torch.int64, device="cuda"), dst, torch.tensor(do, dtype=torch.int64, device="cuda"), res)
        recs = eng.frame_results(res)
        calls += 1
        if not _guard_intact(whole, do[-1]): bad.append((framing, "batch", "", "bytes behind the capacity were written"))
        for k, it in enumerate(its):
            r = recs[k]
            p = _note(it["c"], r.flags)
            if r.status != 0: bad.append((it["c"].name, "batch", "", "status %d" % r.status)); continue
            if not bool((dst[do[k] + len(it["out"]):do[k + 1]] == 0xC3).all()): bad.append((it["c"].name, "batch", "", "bytes behind the frame's content were written"))
            if r.size != len(it["out"]) or not torch.equal(dst[do[k]:do[k] + len(it["out"])], it["exp"]):
                bad.append((it["c"].name, "batch", "", "path %#x size %d: " % (p, r.size) + _explain(it, dst[do[k]:do[k] + min(int(r.size), len(it["out"]))].cpu().numpy().tobytes())))
            if not p & BITS["batch"]: bad.append((it["c"].name, "batch", "", "path %#x lacks batch" % p))
    eng.close()
    ROUTES_RUN.add(5)
    _report("decompress_frames_async, a batch per framing", "", calls, t0, bad)


def test_every_aimed_path_was_seen():
    """Run with the whole file: the route tests record what they saw."""
    want = {1, 5} | {(2, i) for i in range(len(ENVS))} | {(3, n) for n, _ in IX_ENVS} | {(4, "default"), (4, "trace_always")}
    assert ROUTES_RUN == want, ("run the whole file", sorted(map(str, want - ROUTES_RUN)))
    for fam, aims in AIMS.items():
        print("match deps, %-7s path bits seen: %s" % (fam, " ".join(sorted(SEEN.get(fam, ())))))
    missing = {fam: sorted(aims - SEEN.get(fam, set())) for fam, aims in AIMS.items() if aims - SEEN.get(fam, set())}
    assert not missing, ("path bits aimed at and never seen", missing)
    assert set(AIMS) == {f for f, _ in M.FAMILIES}
