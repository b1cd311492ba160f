"""k_spx_index on planted guesses (tests/spx_cases.py), held to the sequential model and to the plain parse (tests/spx_model.py).

Probe (lz4f_mi355x_debug_spx_index: the unchanged kernel on caller-given device bytes).  Every case's frame, a block per
workgroup as in the engine, twice: with the whole frame readable, and with frame_cap at the last payload's last byte (pt_load16
and pt_load8 then take their byte-by-byte branch at the block's end).  gave_up, spx_stitched, and per block cnt, osz, nr and
every point equal the model's; independently of the model, the device's points satisfy the truth invariants of
test_spx_model_cpu.check_points (tokens of the plain parse, from (0, 0, 0), strictly increasing, to (csize, count, size)) - the
check that catches a wrong output position, which nothing downstream verifies; the words of T behind a block's nr + 1 points, and
the rows of stored and declined blocks, keep their pre-fill.  The cases with density words run with them.

End to end.  Every case through Engine.decompress_frame_async under NO_DENSITY_PROBE (the corpus has no preamble for
k_density_probe, and the kernel then gets no only_if - the slow rule is off), alone, with FEED_ROUND=24 and with NO_SELFFEED
(k_spx_parse's route); the output pre-filled with the complement of the expected bytes.  Bytes, size and consumed are exact.
Path bits: self_index and indexed set and dropped clear EXACTLY when the model does not decline; DECLINED below is the list of
cases it declines, written out - the far sides of the exits and of the rescue budget and nothing else - so no other case may
arrive by fallback, which keeps the byte check from passing vacuously.  NO_SPX once, as a control: the same bytes, no self_index.

Failure messages name the case, the switch set, the first differing point or byte and the model's lane fates.

Measured on the MI355X (62 cases, 26 MB of frames): the probe test 124 runs in 0.35 s (0.19 s in the probe calls); each end-to-end
test 62 calls in 0.15-0.52 s; the module 6-7 s, 4.3 of them building the corpus and the model's verdicts on the host.  DESIGN.md
section 4 ("The stretch self-index on planted guesses") has the sensitivity table."""
import ctypes
import time

import numpy as np
import pytest

import spx_cases as C
import spx_model as S
from lz4_frame_conduit_amd import _ffi
from test_gpu_grammar import DROPPED, PATH
from test_gpu_index_forgery import _guard_intact, _out
from test_spx_model_cpu import check_points

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
ROW = 3 * (S.MAXPT + 1)                          # words of T per block
# the cases k_spx_index declines (valid frames, decoded by the generic kernels): a TRUE lane that gives up has no landing, and the
# stitch declines the frame; the stitching thread's own budget
DECLINED = ["exits/by_pair/longs31", "exits/hops/lane0/seqs2050", "exits/hops/lane1/seqs2050", "rescue/seqs65537"]
DECLINED_WITH_DENSITY_WORDS = DECLINED + ["exits/slow/under"]
NDP = {"LZ4F_MI355X_NO_DENSITY_PROBE": "1"}
ENVS = [("no_density_probe", NDP), ("feed_round24", dict(NDP, LZ4F_MI355X_FEED_ROUND="24")), ("no_selffeed", dict(NDP, LZ4F_MI355X_NO_SELFFEED="1")),
        ("no_spx", dict(NDP, LZ4F_MI355X_NO_SPX="1"))]


class Dev:
    """The corpus on the device, made once: per case the frame, its blocks, the model's verdicts, the expected bytes and their complement."""

    def __init__(self):
        import torch
        self.items = []
        for c, fb, out in C.corpus():
            exp = torch.from_numpy(np.frombuffer(out, dtype=np.uint8).copy()).cuda()
            fr = torch.from_numpy(np.frombuffer(fb + bytes(32), dtype=np.uint8).copy()).cuda()
            self.items.append(dict(c=c, fb=fb, out=out, exp=exp, fill=torch.bitwise_not(exp), fr=fr, blocks=C.payloads(fb),
                                   m=C.verdicts(c, fb), m_plain=C.verdicts(c, fb, None)))


@pytest.fixture(scope="module")
def dev():
    return Dev()


@pytest.fixture(scope="module")
def probe():
    L = _ffi.lib()
    assert hasattr(L, "lz4f_mi355x_debug_spx_index"), "the library does not export the stretch-index probe"

    def run(it, frame_cap):
        """-> (gave_up, stitched, per block dict(stored, gave_up, cnt, osz, nr, points, clean))"""
        blocks, c = it["blocks"], it["c"]
        n = len(blocks)
        off = np.array([o for o, _ in blocks], dtype=np.uint64)
        word = np.array([w for _, w in blocks], dtype=np.uint32)
        cnt, osz, nr = (np.full(n, FILL, dtype=np.uint32) for _ in range(3))
        pts = np.zeros(n * ROW, dtype=np.uint32)
        ctl = np.full(2, FILL, dtype=np.uint32)
        nd = bps = None
        if c.density is not None: nd, bps = (ctypes.c_uint32(v) for v in c.density)
        rc = L.lz4f_mi355x_debug_spx_index(it["fr"].data_ptr(), frame_cap, n, off.ctypes.data, word.ctypes.data, ctypes.addressof(nd) if nd is not None else None,
                                           ctypes.addressof(bps) if bps is not None else None, FILL, cnt.ctypes.data, osz.ctypes.data, nr.ctypes.data, pts.ctypes.data, ctl.ctypes.data)
        assert rc == 0, (c.name, rc)
        res = []
        for b in range(n):
            row = pts[b * ROW:(b + 1) * ROW]
            k = int(nr[b])
            assert k <= S.MAXPT, (c.name, b, k)
            used = 3 * (k + 1) if k else 0
            p = [tuple(int(x) for x in row[3 * i:3 * i + 3]) for i in range(k + 1)] if k else []
            res.append(dict(stored=bool(word[b] >> 31), cnt=int(cnt[b]), osz=int(osz[b]), nr=k, points=p, clean=bool((row[used:] == FILL).all())))
        return int(ctl[0]), int(ctl[1]), res

    return run


def _first_diff(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b: return "point %d: device %s, model %s" % (i, a, b)
    return "%d points, the model has %d" % (len(got), len(want))


def test_probe_every_case_is_the_model_and_the_truth(dev, probe):
    t0, bad, runs, t_gpu = time.time(), [], 0, 0.0
    for it in dev.items:
        c, fb = it["c"], it["fb"]
        last_end = it["blocks"][-1][0] + (it["blocks"][-1][1] & 0x7FFFFFFF)
        for cap in (len(fb), last_end):
            who = "frame_cap %d of %d" % (cap, len(fb))
            t1 = time.time()
            gave_up, stitched, res = probe(it, cap)
            t_gpu += time.time() - t1
            runs += 1
            ms = iter(it["m"])
            want_up = any(m["gave_up"] for m in it["m"])
            if bool(gave_up) != want_up or bool(gave_up) != (c.name in DECLINED_WITH_DENSITY_WORDS):
                bad.append((c.name, who, "gave_up %#x, the model %s declines; lanes: %s" % (gave_up, "" if want_up else "never", S.fates(it["m"][0]))))
            if stitched != sum(m["stitched"] for m in it["m"]):
                bad.append((c.name, who, "spx_stitched %d, the model %d; lanes: %s" % (stitched, sum(m["stitched"] for m in it["m"]), S.fates(it["m"][0]))))
            for b, ((off, w), g) in enumerate(zip(it["blocks"], res)):
                if not g["clean"]: bad.append((c.name, who, "block %d: words of T behind its %d points were written" % (b, g["nr"] + 1 if g["nr"] else 0)))
                if g["stored"]:
                    if (g["cnt"], g["osz"], g["nr"]) != (0, w & 0x7FFFFFFF, 0): bad.append((c.name, who, "stored block %d: cnt %d osz %d nr %d" % (b, g["cnt"], g["osz"], g["nr"])))
                    continue
                m = next(ms)
                g["gave_up"] = g["nr"] == 0
                if (g["cnt"], g["osz"], g["nr"]) != (m["cnt"], m["osz"], m["nr"]) or g["points"] != m["points"]:
                    bad.append((c.name, who, "block %d: cnt %d osz %d nr %d, the model %d %d %d; %s; lanes: %s" % (
                        b, g["cnt"], g["osz"], g["nr"], m["cnt"], m["osz"], m["nr"], _first_diff(g["points"], m["points"]), S.fates(m))))
                try:
                    check_points(c.name, fb[off:off + w], g, "device, " + who)      # (independent of the model)
                except AssertionError as e:
                    bad.append((c.name, who, "block %d against the plain parse: %s; lanes: %s" % (b, e, S.fates(m))))
    print("spx probe: %d runs of %d cases in %.2f s (%.2f s in the probe calls)" % (runs, len(dev.items), time.time() - t0, t_gpu))
    for b in bad[:40]: print("   ", *b)
    assert not bad, (len(bad), bad[:6])


def _engine(monkeypatch, env):
    from lz4_frame_conduit_amd.device import Engine
    for k in {k for _, e in ENVS for k in e}: monkeypatch.delenv(k, raising=False)
    for k, v in env.items(): monkeypatch.setenv(k, v)
    return Engine(0)                                      # (switches are read when an engine is made)


@pytest.mark.parametrize("sw", [n for n, _ in ENVS])
def test_end_to_end_bytes_and_path(monkeypatch, dev, sw):
    import torch
    from lz4_frame_conduit_amd.device import DeviceCodecError
    env = dict(ENVS)[sw]
    eng = _engine(monkeypatch, env)
    t0, bad, t_gpu, by_index = time.time(), [], 0.0, 0
    for it in dev.items:
        c, fb, n = it["c"], it["fb"], len(it["out"])
        whole, back = _out(n)
        back[:] = it["fill"]
        torch.cuda.synchronize()
        t1 = time.time()
        try:
            eng.decompress_frame_async(it["fr"], len(fb), back); r = eng.result()
        except DeviceCodecError as e:
            bad.append((c.name, sw, "error: %s" % e)); continue
        t_gpu += time.time() - t1
        fates = S.fates(it["m_plain"][0])
        p = int(r.flags) >> 12
        if not _guard_intact(whole, n): bad.append((c.name, sw, "bytes behind the capacity were written"))
        if r.size != n or r.consumed != len(fb): bad.append((c.name, sw, "path %#x: size %d consumed %d, expected %d %d; lanes: %s" % (p, r.size, r.consumed, n, len(fb), fates)))
        elif not torch.equal(back, it["exp"]):
            d = torch.nonzero(back != it["exp"]).flatten()
            at = int(d[0])
            bad.append((c.name, sw, "path %#x: %d bytes differ, the first at output position %d: got %#04x, expected %#04x (fill %#04x); lanes: %s" % (
                p, len(d), at, int(back[at]), it["out"][at], it["out"][at] ^ 0xFF, fates)))
        declines = any(m["gave_up"] for m in it["m_plain"])
        if declines != (c.name in DECLINED): bad.append((c.name, sw, "the model's verdict and the written-out list differ"))
        indexed = bool(p & PATH["self_index"]) and bool(p & PATH["indexed"]) and not p & DROPPED
        if sw == "no_spx":
            if p & PATH["self_index"]: bad.append((c.name, sw, "path %#x shows self_index" % p))
        elif indexed == declines:
            bad.append((c.name, sw, "path %#x: the model %s, the frame %s; lanes: %s" % (p, "declines" if declines else "does not decline", "came by the self-index" if indexed else "came by fallback", fates)))
        by_index += indexed
    eng.close()
    print("spx end to end under %s: %d cases in %.2f s (%.2f s in the calls), %d by the self-index" % (sw, len(dev.items), time.time() - t0, t_gpu, by_index))
    for b in bad[:40]: print("   ", *b)
    assert not bad, (len(bad), bad[:6])
    assert by_index == (0 if sw == "no_spx" else len(dev.items) - len(DECLINED))


def test_probe_refuses_arguments_out_of_range():
    L = _ffi.lib()
    f = L.lz4f_mi355x_debug_spx_index
    one = ctypes.c_void_p(16)
    off, word = np.array([7], dtype=np.uint64), np.array([100], dtype=np.uint32)
    w = ctypes.c_uint32(1)
    ok = (one, 1000, 1, off.ctypes.data, word.ctypes.data, None, None, FILL, one, one, one, one, one)
    put = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for i in (0, 3, 4, 8, 9, 10, 11, 12): assert f(*put(i, None)) == 1, i          # a null pointer
    assert f(*put(2, 0)) == 1 and f(*put(2, 4097)) == 1                              # no block; more blocks than the probe takes
    assert f(*put(1, 6)) == 1                                                        # a block that starts behind frame_cap
    assert f(*put(1, (1 << 40) + 1)) == 1                                            # no frame is that long
    assert f(*put(5, ctypes.addressof(w))) == 1 and f(*put(6, ctypes.addressof(w))) == 1      # one density word without the other
