"""The planted match-dependency corpus (tests/match_dep_cases.py) on the CPU: every frame is the recorded one, the sequential
model, lz4_grammar's bookkeeping and liblz4 (the oracle) agree on what it decodes to, every case IS what its name says (its
`want` predicates over the sequences as lz4_index.Parsed reads them back), every frame gets a truthful index, and the constants
the cases are placed on are the ones in csrc/*.cuh.  The analysis functions the predicates use are held to hand-written frames
whose answers are spelled out here.

Measured: 337 cases, 37.6 MB decoded; the module takes 42 s on one core (most of it building the corpus and its predicates)."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import lz4_grammar as G
import lz4_index as X
import match_dep_cases as M
import oracle

sha = lambda b: hashlib.sha256(b).hexdigest()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lz4_frame_conduit_amd", "csrc")


@pytest.fixture(scope="module")
def corpus():
    return M.corpus()


def test_frames_are_the_recorded_ones(corpus):
    with open(M.FIXTURE) as f:
        rec = json.load(f)["cases"]
    names = [c.name for c, _, _ in corpus]
    assert len(set(names)) == len(names), "case names repeat"
    assert sorted(names) == sorted(rec), (sorted(set(names) ^ set(rec))[:10], "regenerate with: python -m match_dep_cases")
    for c, fb, out in corpus:
        assert sha(fb) == rec[c.name]["frame_sha256"], (c.name, "the generator no longer makes the recorded frame")
        assert sha(out) == rec[c.name]["out_sha256"], c.name
    total = sum(len(o) for _, _, o in corpus)
    by = {}
    for c, _, o in corpus: by[c.framing] = by.get(c.framing, 0) + 1
    print("match-dependency corpus: %d cases, %d bytes decoded, %d bytes of frames; per framing %s" % (len(corpus), total, sum(len(f) for _, f, _ in corpus), by))
    assert 200 <= len(corpus) and total <= 48 << 20, (len(corpus), total)
    assert by.get("l4m", 0) <= 3 and set(by) == {"i64", "i256", "i4m", "l64", "l256", "l4m"}, by
    assert {c.family for c, _, _ in corpus} == {f for f, _ in M.FAMILIES}


def test_model_builder_and_oracle_agree(corpus):
    for c, fb, out in corpus:
        assert out == bytes(c.fr.out), (c.name, "the model and lz4_grammar.Frame.out differ")
        ref, used = oracle.decompress_frame(fb, cap=len(out) + 64)
        assert used == len(fb) and ref == out, (c.name, "the oracle differs")


def test_literal_background_is_unique(corpus):
    """No 4-byte window occurs twice in the bytes a case's literals were drawn from."""
    for c, _, _ in corpus:
        d = np.frombuffer(c._pool[:max(c._at, 4)], dtype=np.uint8)
        w = d[:-3].astype(np.uint32) | (d[1:-2].astype(np.uint32) << 8) | (d[2:-1].astype(np.uint32) << 16) | (d[3:].astype(np.uint32) << 24)
        assert len(np.unique(w)) == len(w), c.name


def test_every_case_is_what_it_is_named_for(corpus):
    bad = []
    for c, fb, _ in corpus:
        assert c.want and c.aim, (c.name, "a case without a want or an aim")
        A = M.Analysis(fb)
        for what, fn in c.want:
            if not fn(A, c): bad.append((c.name, what))
    assert not bad, bad[:10]


def test_density_is_what_the_case_says(corpus):
    """The model of k_density_probe against the cases' own claim: a block that starts with the preamble is dense or not as built;
    blocks without one (the small slot cases) are whatever their sequences make them, which is why the GPU test asks the model."""
    n = 0
    for c, fb, _ in corpus:
        if c.framing not in ("i256", "i4m"): continue
        A = M.Analysis(fb)
        has_preamble = len(A.S(0)) > 3 and (int(A.S(0)[0, 2]) == 3000 or (int(A.S(0)[0, 2]), int(A.S(0)[1, 2])) == (64, 6))
        if has_preamble: assert A.probe_dense() == c.dense, c.name; n += 1
    assert n >= 150, n


def test_every_case_gets_a_truthful_index(corpus):
    for c, fb, _ in corpus:
        P = X.Parsed(fb)
        assert X.violations(fb, X.build(fb, P), P) == [], c.name
        assert all(B["out_len"] == P.bs for B in P.blocks[:-1]), (c.name, "a block in the middle is short")


def test_constants_are_the_kernels():
    text = {}
    for fn in os.listdir(CSRC):
        if fn.endswith(".cuh"):
            with open(os.path.join(CSRC, fn)) as f: text[fn] = f.read()
    lines = [l for t in text.values() for l in t.splitlines() if "constexpr" in l or "#define" in l]
    for name, want in M.CONSTANTS.items():
        got = [m.group(1) for l in lines for m in re.finditer(r"\b%s\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\b" % name, l)]
        assert got and all(int(g, 0) == want for g in got), (name, want, got)
    for cfg, ring in M.RINGS.items():
        l = [l for l in lines if re.search(r"struct %s\s*\{" % re.escape(cfg), l)]
        assert len(l) == 1, cfg
        assert int(re.search(r"\bRING = (\d+)", l[0]).group(1)) == ring, (cfg, l[0])
        st = re.search(r"\bSTAGE = ([0-9 \-]+),", l[0]).group(1)
        assert eval(st) == M.STAGES[cfg], (cfg, st)
    # FzOpr<C>::N as the kernel's line computes it from the STAGE values just read, against the module's
    opr = re.search(r"struct FzOpr \{ static constexpr uint32_t N = \(2u \* \(C::STAGE \+ FZ_OVER\) >= (\d+)u\) \? (\d+)u : \(2u \* \(C::STAGE \+ FZ_OVER\) >= (\d+)u\) \? (\d+)u : (\d+)u; \}", text["decode_indexed.cuh"])
    assert opr, "FzOpr's line changed"
    t1, n1, t2, n2, n3 = (int(x) for x in opr.groups())
    for cfg in M.STAGES:
        v = 2 * (M.STAGES[cfg] + M.CONSTANTS["FZ_OVER"])
        assert M.fz_opr_n(cfg) == (n1 if v >= t1 else n2 if v >= t2 else n3), cfg
    assert (M.fz_opr_n("FzCfgS4"), M.fz_opr_n("FzCfgS8"), M.fz_opr_n("FzCfg<8>")) == (1024, 2048, 4096)
    for fn, expr in M.SOURCE_LINES:
        assert expr in text[fn], (fn, expr, "the kernel's text changed: look at the cases placed on it")
    assert M.copy_match_plan(1) == (1023, 1024) and M.copy_match_plan(63) == (1008, 1024) and M.copy_match_plan(64) == (0, 64)
    assert M.copy_match_plan(79) == (0, 64) and M.copy_match_plan(1023) == (0, 1008) and M.copy_match_plan(1025) == (0, 1024)
    assert M.fed_per_slot(30, 4) == 10 and M.fed_per_slot(10, 8) == 8 and M.fed_per_slot(190, 4) == 64 and M.fed_per_slot(189, 4) == 63
    assert M.parser_per_slot((96 << 10) - 1) == 8 and M.parser_per_slot(96 << 10) == 64


# ---- the analysis functions on hand-written frames
def _hand1():
    """One independent 64 KiB block:   sequence  literals  match (destination, length, offset)   source
                                           0         20       (20, 8, 10)                          [10, 18): its own literals
                                           1          4       (32, 8, 12)                          [20, 28): exactly match 0
                                           2          0       (40, 6, 3)                           [37, 40) repeating: match 1's tail
                                           3          2       (48, 8, 30)                          [18, 26): two literals, then match 0
                                           4         12       -"""
    fr = G.Frame(4, rng=np.random.default_rng(1))
    b = fr.block()
    b.s(20, 8, 10).s(4, 8, 12).s(0, 6, 3).s(2, 8, 30).end(12)
    return fr.bytes()


def test_analysis_on_a_hand_written_block():
    fb = _hand1()
    A = M.Analysis(fb)
    assert M.model_frame(fb) == oracle.decompress_frame(fb, cap=200)[0]
    assert [A.m(0, i) for i in range(4)] == [(20, 8, 10, 10, 18), (32, 8, 12, 20, 28), (40, 6, 3, 37, 43), (48, 8, 30, 18, 26)]
    assert list(A.depths()[0]) == [1, 2, 3, 2, 0]
    assert A.slot_deps(0, 64) == {0: [], 1: [0], 2: [1], 3: [0]}
    assert A.slot_deps(0, 2) == {0: [], 1: [0], 2: [], 3: []}                       # slots of two: (0, 1), (2, 3)
    assert [A.resolve(0, i, use_parse=False) for i in range(4)] == [("direct", 1), ("direct", 2), ("overlap", 0), ("straddle", 0)]
    assert list(A.parse_direct(0)) == [True, True, False, False, False]             # 1 lies inside match 0, which the parse remembers as payload-backed
    assert [A.resolve(0, i)[0] for i in range(4)] == ["parse", "parse", "overlap", "straddle"]
    assert A.chain(0) == {2, 3}
    assert [e[0] for e in A.lane_cut(0, 66)] == ["one"] * 5                          # (under 96 payload bytes: never the lanes' path)
    assert M.origins(A, 0, 18, 10) == 2 and M.origins(A, 0, 40, 6) == 2 and M.origins(A, 0, 48, 8) == 2
    assert M.owner(A, 19) == (0, 0, "literal") and M.owner(A, 20) == (0, 0, "match") and M.owner(A, 47) == (0, 3, "literal")


def test_analysis_of_the_lanes_cut():
    """300 literals (two length bytes: one_sequence), three 3-byte tokens, a token with a match-length byte, then enough to keep
    96 payload bytes and 1 KiB of room behind the window."""
    fr = G.Frame(4, rng=np.random.default_rng(2))
    b = fr.block()
    b.s(300, 18, 150).s(0, 6, 100).s(0, 6, 100).s(0, 6, 100).s(4, 19, 50)
    for _ in range(12): b.s(100, 8, 50)
    b.end(12)
    A = M.Analysis(fr.bytes())
    ev = A.lane_cut(0, len(fr.out))
    assert ev[0][:2] == ("one", 0) and ev[0][2]["rel0"] == 3
    assert ev[1][0] == "win" and ev[1][1] == [1, 2, 3]
    assert ev[1][2] == dict(mbytes=18, rounds=[[1, 2, 3]], ordered=[], indep={1: True, 2: True, 3: True}, ends={1: 3, 2: 6, 3: 9})
    assert ev[2][:2] == ("one", 4) and all(e[0] == "one" for e in ev[2:])
    assert [e[0] for e in A.lane_cut(0, 318 + 1023)][:2] == ["one", "one"]          # 1023 bytes of room at the window: the scalar path


def test_analysis_of_the_set_aside_list():
    """Linked, two blocks.  Block 1:  0: 20 bytes across the end of block 0's first sparse sequence (424-byte match | 600 literals)
                                      1: reads match 0's destination    2: reads its own literals    3: reads match 1's destination"""
    fr = G.Frame(4, linked=True, rng=np.random.default_rng(3))
    b = fr.block(); b.sparse(fr.bs - 12); b.end(12)
    b = fr.block()
    b.s(3, 20, 3 + fr.bs - 1022).s(2, 20, 22).s(30, 8, 10).s(1, 20, 59).end(12)
    A = M.Analysis(fr.bytes())
    assert A.m(1, 0)[3:] == (1022 - fr.bs, 1042 - fr.bs)
    assert A.resolve(1, 0) == ("straddle", 0) and A.resolve(1, 2)[0] == "parse"
    assert A.chain(1) == {0, 1, 3}
    assert A.set_aside(1, 64) == ([0, 1, 3], False)
    assert A.set_aside(1, 2) == ([0, 1, 3], False)                                   # 3 sits in the next slot: found through the list
    assert A.set_aside(1, 64, own_front=fr.bs) == ([], False)                        # the block in front is this workgroup's own
