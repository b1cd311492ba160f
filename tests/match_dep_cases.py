"""Match copies planted on the decoders' dependency seams: a corpus of named, valid LZ4 frames, a plain sequential model of
what they decode to, and the analysis that says whether a case is what its name claims (test helper, not a test module).

Every decoder of this library decides for itself when a match may be copied and where its bytes come from.  The rest of the
suite reaches those decisions by chance (real and synthetic data) or aims at parsers and bounds (lz4_grammar.py); this module
places a match ON each seam: the last value a branch accepts and the first it does not.

The model (model_frame) is a sequential LZ4 frame decoder: it walks the size words, and per sequence appends the literals and
copies the match - byte by byte where offset < length, by slice otherwise; linked frames reach 64 KiB back.  It shares no
code with lz4_grammar.Block.s, which tracks the output while a frame is BUILT; tests/test_match_dep_cases_cpu.py holds the
two and oracle.decompress_frame to each other.

The cases reuse lz4_grammar.Frame / Block / lz4_seq.  Literals come from ONE stream per case in which no 4-byte window
occurs twice (encoder_cases.unique_stream, PCG64 seeded by the case name's CRC32), so a match copied from the wrong place or
too early cannot produce the right bytes by accident; the GPU test also fills the output with the complement of what is
expected.  Every frame is valid (final literals, last match >= 12 bytes before the block's end; every block of a linked
frame but the last is full, which the indexed decode of linked frames requires).

Framings, the smallest that reach each kernel (engine.hip, decode_plan / dec_index / dec_indexed / dec_generic):
  i64   independent 64 KiB   mode '1': k_decode_blocks -> wave_decode_block_win (lanes' path, one_sequence); batch: k_bf_blocks
  i256  independent 256 KiB  mode 'f', FzCfg<4>: without an index the stretch self-index (k_copy_selffed<FzCfgS4>) or, dense
                             by k_density_probe (< 24 payload bytes per sequence in a block's first 8 KiB), the relay
                             workgroup (k_decode_blocks_relay; DENSE_MODE=2: wave per block); NO_SPX / NO_SELFINDEX: the fused
                             parser k_decode_blocks_fused<FzCfg<4>>.  With an index: k_copy_selffed<FzCfgS4>; NO_SELFFEED:
                             k_parse_indexed + k_resolve_direct + k_copy_indexed<FzCfg<4>>; TRACE_ALWAYS: k_pd_init/k_pd_round;
                             TRACE_ALWAYS + NO_DOUBLING: k_trace_copy
  i4m   block size id 7, one short block: the same with FzCfg<8> / FzCfgS8
  l64   linked 64 KiB        self-index by a lane per block, k_copy_indexed<FzCfg<4>> in groups of blocks (GROUP_KIB,
                             NO_GROUPS), k_decode_linked (LK_WIN) where the index is refused or switched off, the fused
                             workgroup behind it; batch: k_bf_serial
  l256  linked 256 KiB       the same, groups of 2
  l4m   linked 4 MiB         FzCfg<8>; at most three cases (the first block must be full)
A block of an i256 / i4m case starts with a preamble of 8.5 KiB of payload that decides k_density_probe's verdict: `dense`
cases go to the relay / wave decoders, the others to the self-index and the fused workgroups.

Families (the name's first word), the constants they sit on (CONSTANTS; the CPU test reads them back from csrc/*.cuh):
  period  wave_copy_match: one overlapping match per length behind a non-periodic run (64, need = (k-1)*offset, R)
  slot    fz_copier: dep masks, FZ_MATCH_SET, the fastmask split (16, 1024), match_done over ring slots (RING, slots of 64 / 8)
  window  wave_decode_block_win: tokens per 64-byte window (21), rounds of 64 match bytes, indep against md0, the 96 / 1024
          switch to one_sequence, its 64-byte and 504 edges; RL_EXT_MAX
  direct  k_resolve_direct and the self-fed resolve: literal-run edges, IXR_HOPS, run-length sources, the block in front,
          FzOpr<C>::N
  link    the set-aside list of linked frames (FZ_PEND), its closure, groups
  deep    k_pd_init / k_pd_round / k_trace_copy: chain depth (IXP_JUMPS, IXT_MAX_HOPS), folds, postab's 64, IXT_REGION, IXT_STACK
  ring    offsets 65535 / 65534 / 65472 around output positions 65536, 131072, 196608 (LK_WIN, LK_BIAS, RL_MASK)
Where a list of the issue multiplies out (period: offsets x lengths x 16 alignments) one case holds every length of one
offset and the destination alignment ROTATES: match j of the case lands at (base + j) mod 16, base = case number mod 16,
so the lengths meet the alignments over the family's cases; each case's `want` checks its own.  Lengths a framing cannot
hold (70000 in a 64 KiB block) exist in the bigger framings only.

Each case carries `aim` (the kernels and the seam) and `want`: predicates over the frame's sequences AS READ BACK by
lz4_index.Parsed (Analysis below), so a builder that drifts off its seam fails the CPU test rather than silently testing
something else.  `python -m match_dep_cases` (from tests/) rewrites tests/golden/match_deps.json: names and SHA-256 only.
"""
from __future__ import annotations

import hashlib
import json
import os
import struct
import sys
import zlib

import numpy as np

import lz4_grammar as G
import lz4_index as X
from encoder_cases import unique_stream

KB64 = 65536
# the constants the corpus is placed on: csrc/*.cuh, read back by tests/test_match_dep_cases_cpu.py
CONSTANTS = dict(FZ_MATCH_SET=3, FZ_PEND=32, FZ_OVER=576, IXR_HOPS=6, IXP_JUMPS=8, IXP_ROUNDS=12, IXT_STACK=6, IXT_TB=16,
                 IXT_MAX_HOPS=4096, SPX_LANE_HOPS=2048, IXT_REGION_LOG=12, RL_MASK=131071, RL_EXT_MAX=200, LK_WIN=131072, LK_BIAS=65536)
RINGS = {"FzCfg<8>": 8, "FzCfg<4>": 4, "FzCfgS8": 16, "FzCfgS4": 8}                  # FzCfg*::RING
STAGES = {"FzCfg<8>": 8192, "FzCfg<4>": 2048, "FzCfgS8": 4096 - 576, "FzCfgS4": 2048}    # FzCfg*::STAGE (FzOpr<C>::N comes from it)
FRAMING_CFGS = {"i256": ("FzCfg<4>", "FzCfgS4"), "i4m": ("FzCfg<8>", "FzCfgS8")}        # the copy workgroups' shapes per framing
WAVES = {"i64": 4, "i256": 4, "i4m": 8, "l64": 4, "l256": 4, "l4m": 8}               # waves of the copy workgroup per framing
# literal thresholds in the kernels' text (file, the expression as written): the CPU test looks for each
SOURCE_LINES = [
    ("decode_fused.cuh", "has && vml >= 16 && vml <= 1024 && voff >= vml"),
    ("decode_fused.cuh", "k < lane && ms0 < (int32_t)(dk + mk) && ms1 > (int32_t)dk"),
    ("decode_fused.cuh", "csize < (96u << 10) ? 3u : 6u"),
    ("decode_fused.cuh", "per = per > 64 ? 64u : (per < 8 ? 8u : per)"),
    ("common.cuh", "const uint32_t k = (1024 + offset - 1) / offset"),
    ("common.cuh", "const uint32_t R = (offset >= 1024) ? 1024u : (offset & ~15u)"),
    ("common.cuh", "if (offset < 64) {"),
    ("decode.cuh", "csize - pos >= 96u && cap - op >= 1024u"),
    ("decode.cuh", "is_tok && mdst - off + mlen <= md0"),
    ("decode.cuh", "lit <= WAVE && rel0 + lit <= 504u"),
    ("decode.cuh", "if (mlen <= WAVE) {"),
    ("decode_indexed.cuh", "if ((uint64_t)key + ml <= dmj) {"),
    ("decode_indexed.cuh", "for (uint32_t k = (op + 63u) >> 6; (k << 6) < end; k++) T[k] = i;"),        # the position table: a word per 64 output bytes
    ("decode_indexed.cuh", "postab[(e.dst_off >> 6) + (j >> 6)]"),
    ("decode_indexed.cuh", "(2u * (C::STAGE + FZ_OVER) >= 16384u) ? 4096u : (2u * (C::STAGE + FZ_OVER) >= 8192u) ? 2048u : 1024u"),
]


def fz_opr_n(cfg: str) -> int:
    """FzOpr<C>::N, the self-fed position ring's depth in sequences."""
    v = 2 * (STAGES[cfg] + CONSTANTS["FZ_OVER"])
    return 4096 if v >= 16384 else 2048 if v >= 8192 else 1024


def copy_match_plan(offset: int):
    """(need, R) as wave_copy_match computes them: bytes replicated bytewise before it widens, then the round length."""
    need = 0
    if offset < 64:
        k = (1024 + offset - 1) // offset
        need = (k - 1) * offset
        offset *= k
    return need, (1024 if offset >= 1024 else offset & ~15)


def fed_per_slot(nseq: int, waves: int) -> int:
    """Descriptors per ring slot of the fed copiers (fz_feeder, fz_feeder_parse)."""
    per = (nseq + (waves - 1) - 1) // (waves - 1)
    return 64 if per > 64 else 8 if per < 8 else per


def parser_per_slot(csize: int) -> int:
    """Descriptors per ring slot of the fused parser (fz_parser)."""
    return 8 if csize < (96 << 10) else 64


# ------------------------------------------------------------------------------------------------------------------------
# the model
def _model_block(p: bytes, out: bytearray, floor: int):
    """One compressed block appended to `out`; a match may not start below out[floor]."""
    pos, n = 0, len(p)
    while True:
        tok = p[pos]; pos += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                v = p[pos]; pos += 1; lit += v
                if v != 255: break
        assert pos + lit <= n, "literals run past the payload"
        out += p[pos:pos + lit]; pos += lit
        if pos == n: return
        off = p[pos] | (p[pos + 1] << 8); pos += 2
        ml = tok & 15
        if ml == 15:
            while True:
                v = p[pos]; pos += 1; ml += v
                if v != 255: break
        ml += 4
        src = len(out) - off
        assert off > 0 and src >= floor, "a match starts in front of what exists"
        if off < ml:
            for i in range(ml): out.append(out[src + i])
        else:
            out += out[src:src + ml]


def model_frame(frame: bytes) -> bytes:
    """What a valid LZ4 frame (no dictionary) decodes to."""
    assert struct.unpack_from("<I", frame, 0)[0] == 0x184D2204
    flg = frame[4]
    linked, bck, cck = not (flg >> 5) & 1, (flg >> 4) & 1, (flg >> 2) & 1
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    out = bytearray()
    while True:
        word = struct.unpack_from("<I", frame, pos)[0]; pos += 4
        if word == 0: break
        size = word & 0x7FFFFFFF
        if word >> 31: out += frame[pos:pos + size]
        else: _model_block(frame[pos:pos + size], out, max(0, len(out) - KB64) if linked else len(out))
        pos += size + 4 * bck
    assert pos + 4 * cck == len(frame), "bytes behind the frame"
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------------------
# analysis: what the decoders' rules make of a frame's sequences
class Analysis:
    """Over lz4_index.Parsed: per block b, S(b) = (n, 5) rows (token's payload offset, output position, literals, match
    length, offset), positions relative to the block."""

    def __init__(self, frame: bytes):
        self.frame = frame
        self.P = X.Parsed(frame)
        self.linked, self.bs = self.P.linked, self.P.bs
        self._ix = None
        self._pd = {}

    def S(self, b): return self.P.blocks[b]["seqs"]

    def m(self, b, i):
        """Match i of block b: (destination, length, offset, source start, source end), block-relative (source may be < 0)."""
        at, op, lit, ml, off = (int(x) for x in self.S(b)[i])
        d = op + lit
        return d, ml, off, d - off, d - off + ml

    # -- dependency depth per match: 1 + the deepest match any of its source bytes belongs to (literals: 0)
    def depths(self):
        by = np.zeros(self.P.content, np.int32)
        res = []
        for B in self.P.blocks:
            if B["stored"]: res.append(None); continue
            S, base = B["seqs"], B["out_off"]
            dep = np.zeros(len(S), np.int32)
            for i in range(len(S) - 1):
                d = base + int(S[i, 1] + S[i, 2]); ml, off = int(S[i, 3]), int(S[i, 4])
                src = by[d - off:min(d - off + ml, d)]
                dep[i] = 1 + (int(src.max()) if len(src) else 0)
                by[d:d + ml] = dep[i]
            res.append(dep)
        return res

    # -- ring slots and the dependency masks of fz_copier
    def slot_deps(self, b, per, only=None):
        """{i: [k, ...]}: the earlier matches k of i's slot (i // per) whose destination overlaps i's source, as fz_copier's `dep`
        has it (ms0 < dk + mk and ms1 > dk); `only`: the sequences that are on the chain (default: every match)."""
        S = self.S(b)
        out = {}
        for i in range(len(S) - 1):
            if only is not None and i not in only: continue
            _, _, _, s0, s1 = self.m(b, i)
            ks = []
            for k in range(i - i % per, i):
                if only is not None and k not in only: continue
                dk, mk = self.m(b, k)[:2]
                if s0 < dk + mk and s1 > dk: ks.append(k)
            out[i] = ks
        return out

    # -- k_parse_indexed: matches marked direct by the parse (inside one of the last four payload-backed ranges of the index entry's run)
    def parse_direct(self, b):
        if b in self._pd: return self._pd[b]
        if self._ix is None: self._ix = X.build(self.frame, self.P)
        V = X.View(self._ix)
        S = self.S(b)
        mark = np.zeros(len(S), bool)
        eb, ne = int(V.blocks[b, 2]), int(V.blocks[b, 3])
        for e in V.entries[eb:eb + ne]:
            s0, n = int(e[2]), int(e[3]) & 0xFF
            mem = []
            for i in range(s0, min(s0 + n, len(S))):
                at, op, lit, ml, off = (int(x) for x in S[i])
                if lit: mem = [(op, lit)] + mem[:3]
                if ml:
                    dm = op + lit
                    if ml <= off <= dm and any(dm - off >= o and dm - off + ml <= o + n_ for o, n_ in mem):
                        mark[i] = True; mem = [(dm, ml)] + mem[:3]
        self._pd[b] = mark
        return mark

    # -- k_resolve_direct
    def resolve(self, b, i, use_parse=True):
        """(verdict, hops): 'direct' (source found in the payload after `hops` lookups), 'parse' (marked by the parse itself),
        'overlap', 'straddle', 'runlen', 'hops' (IXR_HOPS lookups were not enough), 'far', 'front' (in front of the first block)."""
        d, ml, off, s0, _ = self.m(b, i)
        if use_parse and self.parse_direct(b)[i]: return "parse", 0
        if ml > off: return "overlap", 0
        cb, hi, cur = b, i, self.S(b)
        for hop in range(CONSTANTS["IXR_HOPS"]):
            if s0 < 0:
                if not self.linked or cb == 0: return "front", hop
                cb -= 1
                B = self.P.blocks[cb]
                s0 += B["out_len"]
                if s0 < 0: return "far", hop
                if B["stored"]: return ("direct", hop + 1) if s0 + ml <= B["out_len"] else ("straddle", hop)
                cur = B["seqs"]; hi = len(cur) - 1
            lo = int(np.searchsorted(cur[:hi + 1, 1], s0, side="right")) - 1
            at, opj, litj, mlj, fj = (int(x) for x in cur[lo])
            dmj = opj + litj
            if s0 + ml <= dmj: return "direct", hop + 1
            if s0 < dmj or s0 + ml > dmj + mlj: return "straddle", hop
            if use_parse and self.parse_direct(cb)[lo]: return "direct", hop + 1
            if mlj > fj: return "runlen", hop
            s0 -= fj; hi = lo
        return "hops", CONSTANTS["IXR_HOPS"]

    def chain(self, b):
        """The sequences of block b whose match stays on the chain in the indexed decode (k_resolve_direct finds no payload source)."""
        return {i for i in range(len(self.S(b)) - 1) if self.resolve(b, i)[0] not in ("direct", "parse")}

    # -- fz_copier's set-aside list in a linked frame, the block in front never ready
    def set_aside(self, b, per, own_front=0):
        """(sequences set aside, in list order; True if the list overflowed FZ_PEND - what follows then waits instead)."""
        on = self.chain(b)
        deps = self.slot_deps(b, per, on)
        pend, order = [], []
        n = len(self.S(b))
        for first in range(0, n, per):
            idx = [i for i in range(first, min(first + per, n)) if i in on]
            defer = set()
            for i in idx:
                d, ml, off, s0, s1 = self.m(b, i)
                if s0 < -own_front or any(s0 < hi and s1 > lo for lo, hi in pend): defer.add(i)
            while True:
                add = {i for i in idx if i not in defer and set(deps[i]) & defer}
                if not add: break
                defer |= add
            if len(pend) + len(defer) > CONSTANTS["FZ_PEND"]: return order, True
            for i in sorted(defer):
                d, ml = self.m(b, i)[:2]
                pend.append((d, d + ml)); order.append(i)
        return order, False

    # -- k_density_probe: which decoder a frame of big independent blocks without an index gets
    def probe_dense(self):
        """True: under 24 payload bytes per sequence over the looks of its 64 lanes (a block's first 8 KiB, less per block from 4
        blocks on), the first sequence of each look left out - the relay / wave decoders take the frame; False: the self-index
        and the fused workgroups."""
        n, st, bt = len(self.P.blocks), 0, 0
        seen = set()
        for lane in range(64):
            b = (lane * n) >> 6
            if b in seen: continue
            seen.add(b)
            B = self.P.blocks[b]
            csz = B["csize"]
            if B["stored"] or csz < 64: continue
            p = self.frame[B["src_off"]:B["src_off"] + csz]
            want = 512 if n >= 64 else 512 * (64 // n) if n >= 4 else 8192
            lim = (csz if csz < want else want) - 16
            pos = seqs = first_end = 0                       # (lengths only, as the kernel walks them)
            while pos < lim and seqs < 2048:
                t = p[pos]; pos += 1
                lit = t >> 4
                if lit == 15:
                    while True:
                        x = p[pos] if pos < lim else 0
                        pos += 1; lit += x
                        if not (x == 255 and pos < lim): break
                pos += lit + 2
                if t & 15 == 15:
                    while True:
                        x = p[pos] if pos < lim and pos < len(p) else 0
                        pos += 1
                        if not (x == 255 and pos < lim): break
                seqs += 1
                if seqs == 1: first_end = pos
            if seqs > 1:
                st += seqs - 1
                bt += min(pos, want + 512) - min(first_end, pos)
        return st != 0 and bt < 24 * st

    # -- wave_decode_block_win: how the lanes' path cuts a payload
    def lane_cut(self, b, cap):
        """Events in decode order: ('win', [sequences], info) for a 64-byte window the lanes take - info: mbytes, rounds (lists of
        sequences copied together), ordered (the ordered loop's), indep {i: bool}, ends {i: lane behind the sequence} - and
        ('one', i, info) for one_sequence - info: rel0 (first literal byte relative to the register window's base)."""
        B = self.P.blocks[b]
        p = self.frame[B["src_off"]:B["src_off"] + B["csize"]] + bytes(8)
        S, csize = B["seqs"], B["csize"]
        idx_of = {int(a): i for i, a in enumerate(S[:, 0])}
        ev, pos, op = [], 0, 0
        wb, nb = -512, None

        def ensure(q):
            nonlocal wb, nb
            if 0 <= q - wb < 504: return
            if nb is not None and 0 <= q - nb < 504: wb = nb; nb = wb + 496
            else:
                near = ((q - wb) & 0xFFFFFFFF) < 504 + 64
                wb = q & ~7; nb = wb + 496 if near else None

        def nx(lane):
            a = pos + lane
            t, e1 = p[a], p[a + 1]
            hdr, lit = (2, 15 + e1) if t >> 4 == 15 else (1, t >> 4)
            easy = (t & 15) != 15 and not (hdr == 2 and e1 == 255) and lane + hdr + lit + 2 <= 64
            return lane + hdr + lit + 2 if easy else 255

        while True:
            if csize - pos >= 96 and cap - op >= 1024:
                mask, s = [], 0
                while True:
                    n = nx(s); mask.append(s); sp = s; s = n
                    if n >= 64: break
                if n > 64: mask.pop(); s = sp
                if mask:
                    ids = [idx_of[pos + l] for l in mask]
                    md0 = self.m(b, ids[0])[0]
                    indep = {i: self.m(b, i)[4] <= md0 for i in ids}
                    ml = [int(S[i, 3]) for i in ids]
                    mincl = np.cumsum(ml); mex = mincl - ml
                    rounds, base, together = [], 0, set()
                    while base < int(mincl[-1]):
                        fits = [k for k in range(len(ids)) if mex[k] >= base and mincl[k] <= base + 64]
                        if not fits: break
                        rounds.append([ids[k] for k in fits])
                        together |= {ids[k] for k in fits if indep[ids[k]]}
                        base = int(mincl[fits[-1]])
                    ends = {idx_of[pos + l]: nx(l) for l in mask}
                    ev.append(("win", ids, dict(mbytes=int(mincl[-1]), rounds=rounds, ordered=[i for i in ids if i not in together], indep=indep, ends=ends)))
                    op = int(S[ids[-1], 1] + S[ids[-1], 2] + S[ids[-1], 3])
                    pos += s
                    continue
            i = idx_of[pos]
            at, sop, lit, ml, off = (int(x) for x in S[i])
            ensure(pos)
            hdr = 1 + (0 if lit < 15 else 1 + (lit - 15) // 255)
            rel0 = pos + hdr - wb
            ev.append(("one", i, dict(rel0=rel0, lit=lit, mlen=ml, in_left=csize - pos, out_left=cap - op)))
            if ml == 0: break
            ensure(pos + hdr + lit)
            op = sop + lit + ml
            pos = int(S[i + 1, 0])
        return ev


# ------------------------------------------------------------------------------------------------------------------------
# the case builder
class Case:
    """A named frame under construction.  `marks`: name -> (block, sequence); `want`: [(what, predicate(Analysis, case))]."""

    def __init__(self, name, bsid, linked=False, pool=KB64, aim="", dense=False):
        self.name, self.aim, self.dense = name, aim, dense
        self.seed = zlib.crc32(name.encode())
        rng = np.random.default_rng(self.seed)
        self.fr = G.Frame(bsid, linked=linked)
        self._pool, self._at = unique_stream(rng, pool).tobytes(), 0
        self.marks, self.want, self.anchors = {}, [], []
        self.may_drop = False                               # deep chains: the hop tracer may hand the frame on (IXT_MAX_HOPS)
        self.spx_long = False                               # over SPX_LANE_HOPS short sequences in a row: the stretch self-index declines the frame
        self.b, self.nb = None, -1

    @property
    def framing(self):
        return ("l" if self.fr.linked else "i") + {4: "64", 5: "256", 7: "4m"}[self.fr.bsid]

    @property
    def family(self): return self.name.split("/")[0]
    @property
    def op(self): return self.b.op
    @property
    def nseq(self): return len(self.b.seqs)

    def lit(self, n):
        assert self._at + n <= len(self._pool), (self.name, "literal pool too small", self._at + n)
        self._at += n
        return self._pool[self._at - n:self._at]

    def blk(self, preamble=True):
        self.b = self.fr.block(); self.nb += 1; self.anchors = []
        if preamble and not self.fr.linked and self.fr.bsid >= 5: self.preamble()
        return self

    def s(self, lit, ml, off, mark=None):
        """One sequence; returns its number in the block."""
        n = lit if isinstance(lit, int) else len(lit)
        assert ml >= 4 and 0 < off <= min(self.b.reach + n, 65535), (self.name, self.nseq, n, ml, off, self.b.reach)
        i = self.nseq
        self.b.s(self.lit(lit) if isinstance(lit, int) else lit, ml, off)
        if mark: self.marks[mark] = (self.nb, i)
        return i

    def end(self, n=12):
        assert self.op + n <= self.fr.bs and len(self.b.body) + n + 3 <= self.fr.bs, (self.name, self.op, len(self.b.body))
        self.b.end(self.lit(n)); self.b = None

    def need(self, what, fn): self.want.append((what, fn))

    # -- fillers
    def preamble(self):
        """The block's first 8.5 KiB of payload, which k_density_probe reads: dense (9 payload bytes per sequence) or not."""
        if self.dense:
            self.s(64, 4, 32)
            while len(self.b.body) < 8704: self.s(6, 8, 40)
        else:
            for _ in range(3): self.s(3000, 40, 1000)

    def filler(self, n, lit=160):
        """n sequences whose match is direct (its source lies in its own literal run); the match ends are kept as `anchors`:
        a source laid across one straddles a match and the next literal run."""
        for _ in range(n):
            self.s(lit, 8, lit // 2)
            self.anchors.append(self.op)

    def filler_to_seq(self, k, lit=160):
        assert self.nseq <= k, (self.name, self.nseq, k)
        self.filler(k - self.nseq, lit)

    def strad(self, lit, ml, back=1, mark=None):
        """A chain match for every decoder: its source starts 2 bytes before the `back`-th last anchor (in the filler's match) and
        runs on into the literals behind it."""
        a = self.anchors[-back]
        return self.s(lit, ml, self.op + lit - (a - 2), mark)

    def cheap(self, target):
        """Long non-overlapping matches up to exactly `target` bytes of block output."""
        while self.op < target:
            rem = target - self.op
            assert rem >= 4, (self.name, rem)
            lit = 8 if rem >= 24 else min(rem - 4, 8)
            reach = min(self.b.reach + lit, 65535)
            ml = min(rem - lit, 60000, reach)
            if 0 < rem - lit - ml < 4: ml -= 4
            if ml < 4: lit, ml = rem - 4, 4
            self.s(lit, ml, min(reach, 65535) if ml <= reach else 1)

    def full(self, tail=12):
        """Close a block at exactly the frame's block size."""
        self.cheap(self.fr.bs - tail); self.end(tail)


# ------------------------------------------------------------------------------------------------------------------------
# families
PERIOD_OFFSETS = list(range(1, 18)) + [31, 32, 33, 62, 63, 64, 65, 66, 79, 80, 127, 128, 129, 255, 256, 511, 1008, 1023, 1024, 1025]


def period_lengths(off, big):
    need, R = copy_match_plan(off)
    up = (need + 63) & ~63                           # below 64 the bytewise loop goes in steps of 64: the rounds of R start there
    L = [4, 15, 16, 17, 63, 64, 65, need - 1, need, need + 1, need + R - 1, need + R, need + R + 1, up + R - 1, up + R, up + R + 1, 1024, 1025, off, off + 1] + ([70000] if big else [])
    out = []
    for v in L:
        if v >= 4 and v not in out: out.append(v)
    return out


def _period():
    framings = [(5, False), (7, False), (5, True), (4, False), (4, True)]
    for n, off in enumerate(PERIOD_OFFSETS):
        for bsid, linked in (framings[0], framings[1 + n % 4]):
            big = bsid >= 5
            c = Case("period/off%d/%s%d/a%d" % (off, "l" if linked else "i", bsid, n % 16), bsid, linked, pool=KB64 + 40000,
                     aim="wave_copy_match (fz_copier's generic copy, one_sequence, k_decode_linked, relay): bytewise below 64, need, rounds of R, the last partial round")
            if linked:
                c.blk(); c.s(40000, 8, 100); c.full()
            c.blk()
            lens = period_lengths(off, big)
            for j, L in enumerate(lens):
                lit = off + 16
                lit += (n + j - (c.op + lit)) % 16
                c.s(lit, L, off, "L%d" % L)
            c.end()

            def chk(A, c, off=off, lens=lens, base=n):
                for j, L in enumerate(lens):
                    b, i = c.marks["L%d" % L]
                    at, op, lit, ml, o = (int(x) for x in A.S(b)[i])
                    if (ml, o) != (L, off) or lit < off or (op + lit) % 16 != (base + j) % 16: return False
                return True
            c.need("every length of the offset behind a literal run that holds the period, alignments rotating", chk)
            yield c


def _slot_patterns():
    """(name, emit(c) -> None).  emit appends the pattern's sequences at the current position and adds the wants.  `anchors` exist."""
    def chain(n):
        def emit(c):
            first = c.strad(3, 24, 2, "c0")
            for k in range(1, n): c.s(3, 24, 27, "c%d" % k)

            def chk(A, c, n=n):
                b, i0 = c.marks["c0"]
                for k in range(1, n):
                    d, ml, off, s0, s1 = A.m(b, i0 + k)
                    dp, mp = A.m(b, i0 + k - 1)[:2]
                    if (s0, s1) != (dp, dp + mp): return False
                dep = A.depths()[b]
                return dep[i0 + n - 1] - dep[i0] == n - 1
            c.need("match i reads exactly match i-1's destination, depth grows by one each", chk)
        return emit

    def fan_in(n):
        def emit(c):
            c.strad(5, 20, 2, "f0")
            for k in range(1, n): c.strad(5, 20, 2 + k % 3, "f%d" % k)
            c.s(5, 25 * n - 5, 25 * n, "t")

            def chk(A, c, n=n):
                b, t = c.marks["t"]
                d, ml, off, s0, s1 = A.m(b, t)
                return s0 == A.m(b, t - n)[0] and s1 == A.m(b, t - 1)[0] + 20 and (A.resolve(b, t)[0] == "straddle")
            c.need("one source spans the destinations of n earlier matches and the literals between", chk)
        return emit

    def fan_out(n):
        def emit(c):
            c.strad(4, 32, 2, "src")
            for k in range(n): c.s(2, 32, 34 * (k + 1), "r%d" % k)

            def chk(A, c, n=n):
                b, i0 = c.marks["src"]
                d0, m0 = A.m(b, i0)[:2]
                return all(A.m(b, i0 + 1 + k)[3:] == (d0, d0 + m0) for k in range(n))
            c.need("n matches read one destination", chk)
        return emit

    def edge(which):
        def emit(c):
            c.strad(4, 40, 2, "k")                     # match k at dk, 40 bytes
            # i: 20 bytes, 24 literals in front: its destination is dk + 64.  Both are single-round copies (16..1024 bytes, offset >=
            # length), so they share a register set as soon as the predicate does not order them - only then does a wrong edge show
            off = {"ms0==dk+mk": 24, "ms0==dk+mk-1": 25, "ms1==dk": 84, "ms1==dk+1": 83}[which]
            c.s(24, 20, off, "i")

            def chk(A, c, which=which):
                b, k = c.marks["k"]; i = c.marks["i"][1]
                dk, mk = A.m(b, k)[:2]
                s0, s1 = A.m(b, i)[3:]
                rel = {"ms0==dk+mk": s0 == dk + mk, "ms0==dk+mk-1": s0 == dk + mk - 1, "ms1==dk": s1 == dk, "ms1==dk+1": s1 == dk + 1}[which]
                dep = k in A.slot_deps(b, 1 << 20)[i]
                fast = all(16 <= A.m(b, x)[1] <= 1024 and A.m(b, x)[2] >= A.m(b, x)[1] for x in (k, i))
                return rel and fast and dep == (which in ("ms0==dk+mk-1", "ms1==dk+1"))
            c.need("the dependency predicate's edge " + which, chk)
        return emit

    def split(vml, d):
        def emit(c):
            c.strad(4, vml, 9, "a")                    # a fast or slow match A (its source far back: several anchors)
            c.s(0, vml, vml - d, "b")                  # B reads A's destination: voff = vml - d
            c.s(0, vml, vml, "c")                      # C reads B's
            c.s(3, 16, 3 + 2 * vml, "d")               # D (fast) reads the head of B's destination

            def chk(A, c, vml=vml, d=d):
                b, i = c.marks["b"]
                _, ml, off, s0, s1 = A.m(b, i)
                da, ma = A.m(b, i - 1)[:2]
                return (ml, off) == (vml, vml - d) and s0 == da + d and A.m(b, i + 1)[3] == A.m(b, i)[0] and A.m(b, i + 2)[3] == A.m(b, i)[0]
            c.need("a chain through vml = %d, voff = vml - %d (fast: 16 <= vml <= 1024 and voff >= vml)" % (vml, d), chk)
        return emit

    def ready(n):
        def emit(c):
            for k in range(n): c.strad(2, 48, 2 + k, "p%d" % k)          # n fast matches with nothing in the slot to wait for
            c.s(2, 48 * n + 2 * (n - 1), 48 * n + 2 * (n - 1) + 2, "all")  # and one that waits for all of them

            def chk(A, c, n=n):
                b, t = c.marks["all"]
                deps = A.slot_deps(b, 1 << 20)
                return all(deps[t - n + k] == [] or min(deps[t - n + k]) < t - n for k in range(n)) and [k for k in deps[t] if k >= t - n] == list(range(t - n, t))
            c.need("%d matches ready at once (FZ_MATCH_SET = 3 per register set), then one that reads them all" % n, chk)
        return emit

    pats = []
    # the third entry: how many of the pattern's sequences lie in front of a boundary it is laid across
    for n in (2, 3, 4, 6, 7, 63, 64, 65, 129): pats.append(("chain%d" % n, chain(n), min(n // 2, 30)))
    for n in (2, 3, 4, 5): pats.append(("fanin%d" % n, fan_in(n), n))                    # (the sources in front, their reader behind)
    for n in (4, 7, 64): pats.append(("fanout%d" % n, fan_out(n), 1 + n // 2))           # (the source and half of its readers in front)
    for w in ("ms0==dk+mk", "ms0==dk+mk-1", "ms1==dk", "ms1==dk+1"): pats.append(("edge/" + w, edge(w), 1))
    for vml in (15, 16, 1024, 1025):
        for d in (1, 0): pats.append(("split/vml%d/voff-%d" % (vml, d), split(vml, d), 2))   # (A, B | C, D)
    for n in (4, 7, 8): pats.append(("ready%d" % n, ready(n), n))                         # (the ready ones in front, their reader behind)
    return pats


def _slot():
    aim = "fz_copier (k_decode_blocks_fused, k_copy_indexed, k_copy_selffed): dep_lo/dep_hi, out-of-order replay, fastmask, match_done across ring slots"
    # a boundary placement puts the pattern ACROSS the boundary between slot s - 1 and s: `front` of its sequences in slot s - 1.
    # ringN is the wrap of a descriptor ring of N slots; a framing gets it only where N is a multiple of a RING of its kernels
    # (i256: FzCfg<4> 4, FzCfgS4 8; i4m: FzCfg<8> 8, FzCfgS8 16)
    places = [("mid", None), ("s0|s1", 64), ("ring4", 64 * 4), ("ring8", 64 * 8), ("ring16", 64 * 16)]
    for n, (pname, emit, front) in enumerate(_slot_patterns()):
        for where, boundary in (places[0], places[1 + n % 4]):
            start = 64 * 2 + 5 if boundary is None else boundary - front
            bsid = 7 if n % 3 == 0 and where in ("s0|s1", "ring8", "ring16") else 5
            c = Case("slot/%s/%s/i%d" % (pname, where, bsid), bsid, pool=4 * KB64, aim=aim)
            c.blk()
            pre = c.nseq
            c.filler_to_seq(start)
            emit(c)
            while c.nseq < 620 or len(c.b.body) < 100000: c.filler(1)
            c.end()
            first_mark = min(v[1] for v in c.marks.values())

            def chk(A, c, start=start, first_mark=first_mark):
                b = 0
                B = A.P.blocks[b]
                n = len(A.S(b))
                return first_mark == start and parser_per_slot(B["csize"]) == 64 and fed_per_slot(n, WAVES[c.framing]) == 64
            c.need("the pattern starts at sequence %d of a block whose slots hold 64 descriptors, parsed and fed" % start, chk)
            if boundary is not None:
                last_mark = max(v[1] for v in c.marks.values())

                def crosses(A, c, boundary=boundary, lo=first_mark, hi=last_mark, ring=where):
                    if not lo < boundary <= hi: return False
                    if ring.startswith("ring") and not any(int(ring[4:]) % RINGS[k] == 0 for k in FRAMING_CFGS[c.framing]): return False
                    deps = A.slot_deps(0, 1 << 20)
                    inside = [(i, k) for i in range(lo, hi + 1) for k in deps[i] if k >= lo]
                    return not inside or any(k < boundary <= i for i, k in inside)        # (a pattern without a dependency: its pair on both sides)
                c.need("the pattern lies across sequence %d: a reader behind the boundary, its source in front" % boundary, crosses)
            yield c
        # the same in a small block: slots of 8 (parser) and of 8..64 by the sequence count (fed)
        c = Case("slot/%s/small/i5" % pname, 5, pool=KB64, aim=aim + "; small blocks: shorter slots")
        c.blk(preamble=False)
        c.filler(10)
        emit(c)
        c.filler(3)
        c.end()
        c.need("a block of under 96 KiB of payload: parser slots of 8", lambda A, c: parser_per_slot(A.P.blocks[0]["csize"]) == 8 and fed_per_slot(len(A.S(0)), 4) < 64)
        yield c
    # a slot with only direct matches and literals between two slots with chain matches
    for bsid in (5, 7):
        c = Case("slot/direct_between/i%d" % bsid, bsid, pool=4 * KB64, aim=aim + "; a slot without a chain match neither waits nor is waited for")
        c.blk()
        c.filler_to_seq(64 * 3 - 4)
        c.strad(3, 40, 2, "x")
        c.filler_to_seq(64 * 4 + 3)
        c.s(3, 40, c.op + 3 - c.b.seqs[c.marks["x"][1]][1] - 3, "y")       # reads x's destination, two slots later
        while c.nseq < 620 or len(c.b.body) < 100000: c.filler(1)
        c.end()

        def chk(A, c):
            b, x = c.marks["x"]; y = c.marks["y"][1]
            on = A.chain(b)
            return x // 64 + 2 == y // 64 and not any(i in on for i in range((x // 64 + 1) * 64, (x // 64 + 2) * 64)) and A.m(b, y)[3] == A.m(b, x)[0] and {x, y} <= on
        c.need("chain match, a whole slot of direct matches, a chain match that reads the first", chk)
        yield c


def _window():
    aim = "wave_decode_block_win (k_decode_blocks, k_bf_blocks): tokens per window, rounds of 64 match bytes, indep against md0, the ordered loop, one_sequence"

    def start(name, extra_aim=""):
        c = Case("window/" + name, 4, pool=KB64, aim=aim + extra_aim)
        c.blk()
        c.s(300, 18, 150)                               # something to copy from: 300 literals (a one_sequence: 2 length bytes)
        return c

    def finish(c):
        c.s(40, 4, 20)
        c.filler(14, 100)
        c.end()
        return c

    def toks(c, specs, mark="w"):
        """Easy tokens (lit, mlen <= 18, off) one behind the other; the first is marked."""
        for k, (lit, ml, off) in enumerate(specs): c.s(lit, ml, off, mark if k == 0 else None)

    def win_of(A, c, mark="w"):
        b, i = c.marks[mark]
        for e in A.lane_cut(b, A.P.content):
            if e[0] == "win" and e[1][0] == i: return e
        return None

    # windows of 1, 2, 20, 21 tokens.  A window's last token is taken back when it does not end inside the 64 bytes; a token with
    # a match-length byte (mlen >= 19) is never a lane's.
    for ntok in (1, 2, 20, 21):
        c = start("tokens%d" % ntok)
        c.s(5, 19, 40)                                   # one_sequence: the window behind starts at a token
        if ntok <= 2: specs = [(20, 8, 30)] * ntok + [(30, 19, 50)]          # then a token that is nobody's (mlen 19)
        else: specs = [(0, 6, 100)] * (ntok - 1) + [(64 - 3 * ntok, 6, 100)] + [(4, 19, 50)]
        toks(c, specs)
        finish(c)
        c.need("a window of exactly %d tokens" % ntok, lambda A, c, ntok=ntok: (lambda e: e is not None and len(e[1]) == ntok)(win_of(A, c)))
        yield c
    # match bytes per window, a match straddling each round cut
    for mb in (63, 64, 65, 127, 128, 129):
        n = -(-mb // 18)
        lens = [18] * (n - 1) + [mb - 18 * (n - 1)]
        if lens[-1] < 4: lens[-2] -= 4 - lens[-1]; lens[-1] = 4
        c = start("mbytes%d" % mb)
        c.s(5, 19, 40)
        toks(c, [(1, L, 200) for L in lens] + [(4, 19, 50)])
        finish(c)

        def chk(A, c, mb=mb, n=n):
            e = win_of(A, c)
            if e is None or len(e[1]) != n or e[2]["mbytes"] != mb or e[2]["ordered"]: return False
            cuts = np.cumsum([len(r) for r in e[2]["rounds"]])
            ends = np.cumsum([A.m(0, i)[1] for i in e[1]])
            # every round but the last stops in front of a match that would cross its 64 bytes
            return sum(len(r) for r in e[2]["rounds"]) == n and (len(e[2]["rounds"]) >= 2) == (mb > 64) and all(ends[k] - (ends[cuts[r - 1] - 1] if r else 0) > 64 for r, k in enumerate(cuts[:-1]))
        c.need("%d match bytes in one window, every match in a round" % mb, chk)
        yield c
    # a source ending at md0 - 1, md0, md0 + 1 (the window's first match destination): copied with the rounds, or in order
    for d in (-1, 0, 1):
        c = start("md0%+d" % d)
        c.s(5, 19, 40)
        # tokens: first (lit 6, match 8); second (lit 2, match 8): its destination is md0 + 8 + 2; source end = md0 + d
        toks(c, [(6, 8, 100), (2, 8, 18 - d), (1, 6, 90), (4, 19, 50)])
        finish(c)

        def chk(A, c, d=d):
            e = win_of(A, c)
            if e is None: return False
            b, i = c.marks["w"]
            md0 = A.m(b, i)[0]
            return A.m(b, i + 1)[4] == md0 + d and e[2]["indep"][i + 1] == (d <= 0) and ((i + 1) in e[2]["ordered"]) == (d > 0)
        c.need("a source that ends at md0%+d" % d, chk)
        yield c
    # where the source lies: the window's own literals, the previous window's output, an earlier match of the window
    for kind in ("own_literals", "first_literals", "prev_window", "earlier_match", "earlier_match_overlap", "self_overlap"):
        c = start("source/" + kind)
        c.s(5, 19, 40)
        prev = c.op
        toks(c, [(0, 6, 100)] * 6, "prev")               # a window of six tokens in front,
        c.s(4, 19, 50)                                   # closed by a token that is nobody's
        w = c.op                                         # the window under test: its first token has 12 literals and a 12-byte match
        c.s(12, 12, 100, "w")
        md0 = w + 12
        if kind == "own_literals": c.s(10, 8, 9)
        elif kind == "first_literals": c.s(2, 8, c.op + 2 - (w + 2))
        elif kind == "prev_window": c.s(2, 8, c.op + 2 - (prev + 3))
        elif kind == "earlier_match": c.s(2, 8, c.op + 2 - (md0 + 2))
        elif kind == "earlier_match_overlap": c.s(0, 10, 4)
        else: c.s(5, 12, 3)
        toks(c, [(1, 5, 77), (4, 19, 50)], "tail")
        finish(c)

        def chk(A, c, kind=kind):
            b, i = c.marks["w"]
            e = win_of(A, c)
            ep = win_of(A, c, "prev")
            if e is None or ep is None or len(ep[1]) != 6 or e[1][:2] != [i, i + 1]: return False
            d, ml, off, s0, s1 = A.m(b, i + 1)
            md0, m0 = A.m(b, i)[:2]
            w0, own = int(A.S(b)[i, 1]), int(A.S(b)[i + 1, 1])
            p0 = int(A.S(b)[ep[1][0], 1])
            where = {"own_literals": own <= s0 and s1 <= d, "first_literals": w0 <= s0 and s1 <= md0, "prev_window": p0 <= s0 and s1 <= p0 + 36,
                     "earlier_match": md0 <= s0 and s1 <= md0 + m0 and off >= ml, "earlier_match_overlap": md0 <= s0 < md0 + m0 and off < ml,
                     "self_overlap": own <= s0 and off < ml}[kind]
            return where and e[2]["indep"][i + 1] == (kind in ("first_literals", "prev_window")) and ((i + 1) in e[2]["ordered"]) == (kind not in ("first_literals", "prev_window"))
        c.need("the second token's source: " + kind + " (with the rounds if it ends at or below md0, else in the ordered loop)", chk)
        yield c
    # a sequence whose last byte is lane 62, 63 or 64 of the window
    for last in (62, 63, 64):
        c = start("lastlane%d" % last)
        c.s(5, 19, 40)
        toks(c, [(10, 6, 100), (last - 16, 7, 60), (3, 5, 30), (4, 19, 50)])     # (lanes 0..12; 13: token, length byte, literals, offset)
        finish(c)

        def chk(A, c, last=last):
            e = win_of(A, c)
            if e is None: return False
            i = c.marks["w"][1]
            return (len(e[1]) == 2 and e[2]["ends"][i + 1] == last + 1) if last < 64 else (len(e[1]) == 1)
        c.need("the second sequence's last payload byte is lane %d: inside the window up to 63" % last, chk)
        yield c
    # one literal-length byte
    for L in (15, 269, 270):
        c = start("litbyte%d" % L)
        c.s(5, 19, 40)
        toks(c, [(3, 6, 100), (L, 6, 50), (2, 5, 30), (4, 19, 50)])
        finish(c)
        c.need("a literal run of %d bytes behind an easy token" % L, lambda A, c, L=L: int(A.S(0)[c.marks["w"][1] + 1, 2]) == L)
        yield c
    # match lengths around the nibble (18 / 19) and RL_EXT_MAX (218 / 219 / 220)
    for M in (18, 19, 218, 219, 220):
        for dense in (False, True):
            if dense:
                c = Case("window/mlen%d/relay" % M, 5, pool=KB64, dense=True, aim="k_decode_blocks_relay: tokens with one match-length byte up to RL_EXT_MAX stay in the lanes")
                c.blk()
            else:
                c = start("mlen%d" % M); c.s(5, 19, 40)
            for rep in range(3):
                toks(c, [(3, 6, 100), (2, M, 300), (1, 5, 30)], "w%d" % rep)
                if dense: c.s(6, 8, 40)
            if dense:
                for _ in range(200): c.s(6, 8, 40)
            finish(c)
            c.need("matches of %d bytes" % M, lambda A, c, M=M: all(int(A.S(0)[c.marks["w%d" % r][1] + 1, 3]) == M for r in range(3)))
            yield c
    # the scalar fallback's edges: csize - pos in {95, 96} and cap - op in {1023, 1024} at a token that would be a window's first
    for gap in (95, 96):
        c = start("csize-pos%d" % gap)
        c.s(5, 19, 40)
        c.s(2, 6, 100, "w")
        # behind w's token `gap` payload bytes in all: w (5), an easy token (4), a long match (9: cap - op stays >= 1024), final literals
        c.s(1, 6, 100); c.s(1, 1100, 200)
        c.end(gap - 18 - 2)                              # token + one length byte + literals (15 <= n < 270)
        c.need("csize - pos == %d at a token" % gap, lambda A, c, gap=gap: A.P.blocks[0]["csize"] - int(A.S(0)[c.marks["w"][1], 0]) == gap and
               any(e[0] == "win" and e[1][0] == c.marks["w"][1] for e in A.lane_cut(0, A.P.content)) == (gap == 96))
        yield c
    for gap in (1023, 1024):
        c = start("cap-op%d" % gap)
        c.s(5, 19, 40)
        c.s(2, 6, 100, "w")
        c.s(1, 6, 100); c.s(1, 6, 100)
        tail = gap - 8 - 14
        c.s(tail - 200 - 4, 4, 9)
        c.end(200)
        c.need("cap - op == %d at a token (capacity = content)" % gap, lambda A, c, gap=gap: A.P.content - int(A.S(0)[c.marks["w"][1], 1]) == gap and
               any(e[0] == "win" and e[1][0] == c.marks["w"][1] for e in A.lane_cut(0, A.P.content)) == (gap == 1024))
        yield c
    # one_sequence: a byte per lane up to 64; literals out of the register window up to rel0 + lit <= 504
    for M in (64, 65):
        c = start("one/mlen%d" % M)
        for off in (M, M - 1, 7, 300): c.s(5, M, off, "w" if off == M else None)
        finish(c)
        c.need("one_sequence with matches of %d bytes, overlapping and not" % M, lambda A, c, M=M: all(e[0] == "one" for e in A.lane_cut(0, A.P.content) if e[1] == c.marks["w"][1]) and int(A.S(0)[c.marks["w"][1], 3]) == M)
        yield c
    for L in (64, 65):
        c = start("one/lit%d" % L)
        c.s(L, 19, 30, "w"); c.s(L, 19, L + 1)
        finish(c)
        c.need("one_sequence with %d literals" % L, lambda A, c, L=L: any(e[0] == "one" and e[1] == c.marks["w"][1] and e[2]["lit"] == L for e in A.lane_cut(0, A.P.content)))
        yield c
    for edge in (504, 505):
        c = Case("window/one/rel0+lit%d" % edge, 4, pool=KB64, aim=aim + "; literals served from the register window")
        c.blk()
        # one_sequence tokens from the block's first byte: the window's base stays 0 until a read at 504 or beyond
        while len(c.b.body) + 16 < 470: c.s(10, 19, 5)
        rel0 = len(c.b.body) + 2                         # token, one length byte
        c.s(edge - rel0, 19, 30, "w")
        finish(c)
        c.need("rel0 + lit == %d" % edge, lambda A, c, edge=edge: any(e[0] == "one" and e[1] == c.marks["w"][1] and e[2]["rel0"] + e[2]["lit"] == edge and e[2]["lit"] <= 64 for e in A.lane_cut(0, A.P.content)))
        yield c


def _direct():
    aim = "k_resolve_direct / fz_feeder_parse's resolve (k_copy_indexed, k_copy_selffed): literal-run edges, IXR_HOPS, run-length sources, FzOpr<C>::N"

    def base(name, bsid=5, linked=False, pool=KB64 + 20000):
        c = Case("direct/" + name, bsid, linked, pool=pool, aim=aim)
        c.blk()
        c.filler(40)
        return c

    def close(c):
        c.filler(20); c.end()
        return c

    # sources against a literal run [r0, r1) that is 6 sequences back (out of the parse's own memory of four ranges)
    for bsid in (5, 7):
        for kind in ("first_byte", "last_byte", "past_last", "before_first"):
            c = base("litrun/%s/i%d" % (kind, bsid), bsid)
            r = c.s(120, 8, 60, "run")                   # the run: 120 literals
            r0 = c.op - 8 - 120
            c.filler(6)
            s0 = {"first_byte": r0, "last_byte": r0 + 120 - 16, "past_last": r0 + 120 - 15, "before_first": r0 - 1}[kind]
            c.s(4, 16, c.op + 4 - s0, "t")
            close(c)

            def chk(A, c, kind=kind):
                b, t = c.marks["t"]
                v = A.resolve(b, t)
                return v == (("direct", 1) if kind in ("first_byte", "last_byte") else ("straddle", 0))
            c.need("16 bytes from a literal run's %s: direct only while wholly inside" % kind, chk)
            yield c
    # hop depth: t reads inside M_d, which reads M_(d-1) shifted by one byte across a literal (a straddle: stays on the chain in
    # every kernel), ... down to M_1, whose source is a literal run
    for d in range(1, 9):
        for bsid in ((5, 7) if d in (5, 6, 7) else (5,)):
            c = base("hops%d/i%d" % (d, bsid), bsid)
            zs = c.op
            c.s(100, 8, 50)
            c.filler(6)
            c.s(1, 40, c.op + 1 - (zs + 10), "m1")                  # M_1: 40 bytes out of the 100 literals, 7 sequences back
            for k in range(2, d + 1): c.s(1, 40, 40, "m%d" % k)
            c.filler(6)
            md = c.b.seqs[c.marks["m%d" % d][1]]
            c.s(3, 8, c.op + 3 - (md[1] + md[2]), "t")              # the first 8 bytes of M_d
            close(c)

            def chk(A, c, d=d):
                b, t = c.marks["t"]
                v = A.resolve(b, t)
                ok_mid = all(A.resolve(b, c.marks["m%d" % k][1])[0] == "straddle" for k in range(2, d + 1))
                return ok_mid and v == (("direct", d + 1) if d + 1 <= CONSTANTS["IXR_HOPS"] else ("hops", CONSTANTS["IXR_HOPS"]))
            c.need("a source %d plain matches deep: found in the payload up to IXR_HOPS lookups" % d, chk)
            yield c
    # a source that ends in / lies in a run-length match; one inside a match the parse marked direct
    for kind in ("in_runlen", "ends_in_runlen", "in_parse_direct"):
        c = base(kind)
        if kind == "in_parse_direct":
            c.s(100, 30, 80, "p")
            c.filler(6)
            p = c.b.seqs[c.marks["p"][1]]
            c.s(3, 12, c.op + 3 - (p[1] + p[2] + 5), "t")
        else:
            c.s(20, 90, 7, "rl")
            c.filler(6)
            r = c.b.seqs[c.marks["rl"][1]]
            s0 = r[1] + r[2] + 30 if kind == "in_runlen" else r[1] + r[2] + 90 - 16      # (ends on the run-length match's last byte)
            c.s(3, 16, c.op + 3 - s0, "t")
        close(c)
        want = {"in_runlen": ("runlen", 0), "ends_in_runlen": ("runlen", 0), "in_parse_direct": ("direct", 1)}[kind]
        c.need("source " + kind, lambda A, c, want=want: A.resolve(*c.marks["t"]) == want)
        yield c
    # linked: the source in the block in front - compressed, stored - straddling the boundary, and an overlapping match that starts there
    for bsid in (4, 5):
        for kind in ("front_literals", "front_match", "front_stored", "straddle_boundary", "overlap_from_front"):
            c = Case("direct/linked/%s/l%d" % (kind, bsid), bsid, True, pool=(1 << (8 + 2 * bsid)) + KB64, aim=aim + "; the block in front")
            bs = c.fr.bs
            if kind == "front_stored":
                c.fr.stored(c.lit(bs)); c.nb += 1
            else:
                c.blk(); c.filler(20); c.cheap(bs - 500); c.s(480, 8, 20, "last"); c.end(12)
            c.blk()
            c.s(30, 8, 15)
            if kind == "front_literals": c.s(4, 16, c.op + 4 + 12 + 8 + 300, "t")
            elif kind == "front_match": c.s(4, 8, c.op + 4 + 12 + 8, "t")
            elif kind == "front_stored": c.s(4, 16, c.op + 4 + 1000, "t")
            elif kind == "straddle_boundary": c.s(4, 40, c.op + 4 + 10, "t")
            else: c.s(0, 200, c.op + 5, "t")
            c.filler(20); c.end()
            want = {"front_literals": ("direct", 1), "front_match": ("direct", 1), "front_stored": ("direct", 1), "straddle_boundary": None, "overlap_from_front": ("overlap", 0)}[kind]

            def chk(A, c, kind=kind, want=want):
                b, t = c.marks["t"]
                d, ml, off, s0, s1 = A.m(b, t)
                if s0 >= 0: return False
                if kind == "straddle_boundary": return s1 > 0 and A.resolve(b, t)[0] not in ("direct", "parse")
                if kind == "overlap_from_front": return off < ml and A.resolve(b, t) == want
                return s1 <= 0 and A.resolve(b, t)[0] == "direct"
            c.need("linked, source " + kind, chk)
            yield c
    # a source produced N - 1, N, N + 1 sequences earlier (the self-fed ring of output positions)
    for N in (1024, 2048, 4096):
        for bsid in (5, 7):
            c = Case("direct/opr%d/i%d" % (N, bsid), bsid, pool=KB64, aim=aim + "; FzOpr<C>::N sequences back")
            # (N - 2 sequences of 6 payload bytes in a row.  decode_spx.cuh's stretch lanes give up a chain that crawls - SPX_LANE_HOPS
            # sequences, and a bytes-per-hop test every 64 - so from a run of about SPX_LANE_HOPS on the frame WITHOUT an index is
            # sent to the generic decoders by design: written down here, with the bits the GPU test must then see instead.  The
            # self-fed ring is reached with the index of routes 3 and 4 either way.)
            c.spx_long = N >= CONSTANTS["SPX_LANE_HOPS"]
            c.blk()
            c.filler(4, 60)
            first = c.nseq
            src = c.op
            c.s(60, 8, 20, "src")
            while c.nseq < first + N - 1: c.s(3, 8, 5)
            for k in range(3): c.s(2, 12, c.op + 2 - (src + 4 + 12 * k), "t%d" % k)      # three in a row read the one literal run
            c.filler(4, 60); c.end()

            def chk(A, c, N=N):
                dist = [c.marks["t%d" % k][1] - c.marks["src"][1] for k in range(3)]
                return dist == [N - 1, N, N + 1] and all(A.resolve(0, c.marks["t%d" % k][1], use_parse=False) == ("direct", 1) for k in range(3))
            c.need("sources %d - 1, %d and %d + 1 sequences back" % (N, N, N), chk)
            yield c


def _link():
    aim = "fz_copier's set-aside list in linked frames (k_copy_indexed): FZ_PEND, the closure loop, groups of blocks"

    def reach_front(c, lit, ml, k, mark=None):
        """A chain match of the current block whose source straddles anchor k of the block in front."""
        a = c.prev_anchors[k] - c.fr.bs                   # relative to this block
        return c.s(lit, ml, c.op + lit - (a - 2), mark)

    def begin(name, bsid=4, pool=None):
        c = Case("link/" + name, bsid, True, pool=pool or (3 * KB64), aim=aim)
        c.blk(); c.s(2000, 8, 1000)
        c.cheap(c.fr.bs - 12 - 250 * 208 - 100)
        c.filler(250, 200)
        c.prev_anchors = list(c.anchors)
        c.full()
        return c

    for bsid in (4, 5, 7):
        for nfront in (0, 1, 31, 32, 33, 40):
            for spread in (False, True):
                if bsid == 7 and (nfront, spread) not in ((33, False), (31, True)): continue      # (4 MiB of history each: two cases)
                c = begin("front%d/%s/l%d" % (nfront, "spread" if spread else "one_slot", bsid), bsid)
                c.blk()
                c.filler(70, 100)
                for k in range(nfront):
                    reach_front(c, 2, 20, 200 + k, "f%d" % k)
                    if spread: c.filler(8, 80)
                c.filler(420 if bsid == 7 else 60, 100)      # (eight waves: slots of 64 from 442 sequences on)
                c.end()

                def chk(A, c, nfront=nfront, spread=spread):
                    b = 1
                    per = fed_per_slot(len(A.S(b)), WAVES[c.framing])
                    order, over = A.set_aside(b, per)
                    fr = [i for i in A.chain(b) if A.m(b, i)[3] < 0]
                    slots = {i // per for i in fr}
                    return len(fr) == nfront and over == (nfront > CONSTANTS["FZ_PEND"]) and (nfront < 2 or (len(slots) > 2) == spread) and (over or order == sorted(fr))
                c.need("%d chain matches reach into the block in front (FZ_PEND = 32 fit the list)" % nfront, chk)
                yield c
    # closure: a later chain match reads a set-aside match's destination - directly, through 2 and 3 others; in the slot, in a later slot
    for through in (1, 2, 3):
        for later in (False, True):
            c = begin("closure%d/%s" % (through, "later_slot" if later else "in_slot"))
            c.blk()
            c.filler(70, 100)
            reach_front(c, 2, 24, 210, "a")
            if later: c.filler(70, 100)
            for k in range(through):
                c.s(3, 24, 27 if (k or not later) else c.op + 3 - (c.b.seqs[c.marks["a"][1]][1] + 2), "x%d" % k)
            c.filler(100, 100); c.end()

            def chk(A, c, through=through, later=later):
                b, a = c.marks["a"]
                per = fed_per_slot(len(A.S(b)), 4)
                order, over = A.set_aside(b, per)
                xs = [c.marks["x%d" % k][1] for k in range(through)]
                return not over and order == [a] + xs and ((xs[0] // per != a // per) == later)
            c.need("the set-aside list closes over %d matches that read a set-aside destination" % through, chk)
            yield c
    # three blocks: block 2 reads bytes that block 1 set aside
    for bsid in (4,):
        c = begin("three_blocks/l%d" % bsid, bsid, pool=4 * KB64)
        c.blk(); c.filler(70, 100)
        reach_front(c, 2, 24, 220, "a")
        a_dst = c.op - 24
        c.filler(150, 100)
        c.prev_anchors = [x for x in c.anchors]
        c.full()
        c.blk(); c.filler(30, 100)
        c.s(2, 24, c.op + 2 + (c.fr.bs - a_dst), "r")     # block 2 reads a's destination in block 1
        c.filler(50, 100); c.end()

        def chk(A, c):
            b, r = c.marks["r"]
            a = c.marks["a"][1]
            s0 = A.m(b, r)[3] + A.bs
            return (b, c.marks["a"][0]) == (2, 1) and s0 == A.m(1, a)[0] and a in A.set_aside(1, fed_per_slot(len(A.S(1)), 4))[0] and A.resolve(b, r)[0] not in ("direct", "parse")
        c.need("block 2 reads what block 1 set aside", chk)
        yield c
    # 64 KiB blocks around the group boundary (a group is 512 KiB of blocks by default: 8): the group's first block reads another
    # workgroup's output, the others their own workgroup's; the list is carried and rebased from block to block
    c = begin("groups/l4", 4, pool=12 * KB64)
    for blk in range(1, 11):
        c.blk(); c.filler(70, 100)
        for k in range(3): reach_front(c, 2, 24, 200 + 3 * k, "b%d_%d" % (blk, k))
        c.s(3, 24, 27, "b%d_c" % blk)
        c.filler(160, 100)
        c.prev_anchors = list(c.anchors)
        if blk < 10: c.full()
        else: c.end()
    c.need("ten blocks, each with three chain matches into the block in front and one reading the last of them",
           lambda A, c: len(A.P.blocks) == 11 and all({c.marks["b%d_%d" % (b, k)][1] for k in range(3)} <= {i for i in A.chain(b) if A.m(b, i)[3] < 0} and
                                                      A.m(b, c.marks["b%d_c" % b][1])[3] == A.m(b, c.marks["b%d_2" % b][1])[0] for b in range(1, 11)))
    yield c


def _deep():
    aim = "k_pd_init / k_pd_round (pointer doubling), k_trace_copy (hop tracer), and every chain decoder: copy chains"

    def begin(name, bsid=5, linked=False, pool=KB64):
        c = Case("deep/" + name, bsid, linked, pool=pool, dense=True, aim=aim)
        c.blk()
        return c

    for depth in (1, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097):
        for bsid in ((5, 7) if depth in (8, 4096) else (5,)):
            c = begin("chain%d/i%d" % (depth, bsid), bsid)
            c.may_drop = depth >= 4096
            c.s(24, 8, 17, "m0")                            # depth 1: out of its own literals
            for k in range(1, depth): c.s(1, 8, 9)          # each copies the match in front
            c.marks["t"] = (c.nb, c.nseq - 1)
            c.s(30, 4, 11); c.end()
            c.need("a chain %d matches deep" % depth, lambda A, c, depth=depth: int(A.depths()[0][c.marks["t"][1]]) == depth)
            yield c
    # as deep as a 256 KiB block of minimum-length sequences allows: a literal and a 4-byte match that copies the match in front
    c = begin("longest/i5", pool=KB64 + 8192)
    c.may_drop = True
    c.s(24, 4, 9, "m0")
    while c.op + 5 + 12 + 8 <= c.fr.bs - 64: c.s(1, 4, 5)
    c.marks["t"] = (0, c.nseq - 1)
    c.end()
    c.need("one chain through the whole block", lambda A, c: int(A.depths()[0][c.marks["t"][1]]) == c.marks["t"][1] - c.marks["m0"][1] + 1 >= 45000)
    yield c
    # run-length matches in the middle of a chain
    for off in (1, 2, 3, 7, 9, 63, 64, 65):
        c = begin("fold%d/i5" % off)
        c.s(80, 8, 40)
        for k in range(5): c.s(1, 8, 9)
        c.s(0, 3 * off + 37, off, "rl")                     # replicates the bytes in front of it (the chain's last match for off <= 8)
        rl_end = c.op
        for k in range(12): c.s(1, 10, 11 + 3 * k)            # then a chain that walks back through the run-length match
        c.marks["t"] = (0, c.nseq - 1)
        c.s(30, 4, 11); c.end()

        def chk(A, c, off=off):
            b, r = c.marks["rl"]
            d, ml, o, s0, s1 = A.m(b, r)
            dep = A.depths()[b]
            return o == off and ml > o and dep[c.marks["t"][1]] > dep[r]
        c.need("a run-length match of offset %d inside a chain" % off, chk)
        yield c
    # sequences that start at output positions 63, 64, 65 mod 64 and 4095, 4096, 4097 (the position table, the regions)
    for at in (63, 64, 65, 4095, 4096, 4097):
        c = begin("start%d/i5" % at)
        base = ((c.op + 600) // 4096 + 1) * 4096 if at >= 4095 else ((c.op + 100) // 64 + 1) * 64
        tgt = base + (at % 4096 if at >= 4095 else at - 64)
        while tgt - c.op >= 9 + 4 + 20: c.s(1, 8, 9)
        c.s(tgt - c.op - 4, 4, 9)
        assert c.op == tgt
        for k in range(8): c.s(1, 8, 9, "t" if k == 0 else None)
        c.s(30, 4, 11); c.end()
        c.need("a sequence starts at output position %d (mod %d)" % (at, 4096 if at >= 4095 else 64),
               lambda A, c, at=at: int(A.S(0)[c.marks["t"][1], 1]) % (4096 if at >= 4095 else 64) == at % (4096 if at >= 4095 else 64))
        yield c
    # 16-byte spans (aligned: a tracer thread's) whose bytes have 6, 7 and 16 different origins
    for norig in (6, 7, 16):
        c = begin("origins%d/i5" % norig)
        z = c.op
        c.s(100, 8, 50)                                       # Z: 100 literals
        if norig == 16:
            # P0: literal | 4 bytes of Z.  P1: literal | (P0's last match byte, the next literal, two match bytes): 3 origins.
            # P2: literal | (P1's last match byte, the next literal, two match bytes): 4 origins - so in P2 no two neighbours share one
            for k in range(8): c.s(1, 4, 60)
            for k in range(8): c.s(1, 4, 37)
            p2 = c.op
            for k in range(8): c.s(1, 4, 37)
            span = (p2 + 15) & ~15
        else:
            c.s(16 + (-(c.op + 20)) % 16, 4, 9)               # to a multiple of 16
            span = c.op
            for k in range(3): c.s(1, 5 if (k == 2 and norig == 6) else 4, c.op + 1 - (z + 10))     # literal | a match out of Z, three times,
            c.s(1, 4, c.op + 1 - (z + 30))                    # and the next literal (7 origins) or the match's fifth byte (6)
        c.marks["t"] = (0, c.nseq - 1)
        c.s(30, 4, 11); c.end()
        c.need("an aligned 16-byte span with %d origins" % norig, lambda A, c, norig=norig, span=span: span % 16 == 0 and origins(A, 0, span, 16) == norig)
        yield c


def origins(A: Analysis, b: int, pos: int, n: int) -> int:
    """How many pieces the n output bytes at block position pos fall into when every byte is traced to the literal it comes
    from: neighbours belong to one piece when their origins are neighbours in one literal run (k_trace_copy / k_pd_init)."""
    S = A.S(b)

    def origin(j):
        while True:
            i = int(np.searchsorted(S[:, 1], j, side="right")) - 1
            at, op, lit, ml, off = (int(x) for x in S[i])
            if j < op + lit: return i, j - op
            r = j - (op + lit)
            j = op + lit - off + (r % off if off <= r else r)
    o = [origin(pos + k) for k in range(n)]
    return 1 + sum(1 for k in range(1, n) if not (o[k][0] == o[k - 1][0] and o[k][1] == o[k - 1][1] + 1))


def _ring():
    aim = "k_decode_linked (LK_WIN, LK_BIAS), k_decode_blocks_relay (RL_MASK): sources and destinations across the 64 KiB wraps"
    for bsid, linked in ((5, False), (4, True), (5, True)):
        for P, v in ((P, v) for P in (65536, 131072, 196608) for v in range(3)):
            # matches that cross one wrap land on top of each other, so each case holds one of three sets:
            #   v0  destination across P (65472), source across P (65472), source across P and destination across P + 64 KiB (65535)
            #   v1  destination across P (65534), both (65534)
            #   v2  destination across P (65535), a source that starts one byte before P (65535)
            bs = 1 << (8 + 2 * bsid)
            if v == 0: plan = [(P - 8, 32, 65472, "dst"), (P - 8 + 65472, 32, 65472, "src"), (P - 9 + 65535, 40, 65535, "both")]
            elif v == 1: plan = [(P - 12, 40, 65534, "dst"), (P - 20 + 65534, 48, 65534, "both")]
            else: plan = [(P - 30, 44, 65535, "dst"), (P - 1 + 65535, 30, 65535, "both")]
            plan = [x for x in plan if x[0] >= x[2] + 64]     # (absolute destination, length, offset, mark); the source exists
            # a match lives in one block and ends 17 bytes before its end at the latest (in i256 and l256 the wraps lie inside a block,
            # in l64 they are the block boundaries: there only sources cross them)
            plan = sorted(x for x in plan if x[0] // bs == (x[0] + x[1] + 17) // bs and (linked or x[0] + x[1] + 17 < bs))
            if not plan: continue
            c = Case("ring/%s%d/at%d/v%d" % ("l" if linked else "i", bsid, P, v), bsid, linked, pool=5 * KB64, dense=not linked, aim=aim)
            for d, ml, off, mark in plan:
                # up to d: literals mostly (what the matches copy must be unique bytes), in sequences of 3000
                while True:
                    if c.b is None: c.blk()
                    pos, blk_end = len(c.fr.out), (c.nb + 1) * bs
                    if d >= blk_end:                           # the match belongs to a later block: this one is filled to its end
                        while blk_end - len(c.fr.out) > 3100: c.s(2000, 1000, 1500)
                        c.full()
                        continue
                    if d - pos <= 3016: break
                    c.s(2000, 1000, 1500)
                c.s(d - pos, ml, off, mark)
            if (c.nb + 1) * bs - len(c.fr.out) < 200: c.full()
            else: c.s(100, 4, 50); c.end()

            def chk(A, c, P=P, plan=plan):
                for d, ml, off, mark in plan:
                    b, i = c.marks[mark]
                    dd, mml, o = A.m(b, i)[:3]
                    if (dd + A.P.blocks[b]["out_off"], mml, o) != (d, ml, off): return False
                return True
            c.need("matches of offsets 65535 / 65534 / 65472 whose source, destination or both cross %d (+ 64 KiB)" % P, chk)
            yield c


FAMILIES = [("period", _period), ("slot", _slot), ("window", _window), ("direct", _direct), ("link", _link), ("deep", _deep), ("ring", _ring)]


def cases(families=None):
    """Every case, built: a generator of Case (frame bytes: case.fr.bytes(); expected output: model_frame of them)."""
    for fam, gen in FAMILIES:
        if families is None or fam in families:
            yield from gen()


_CORPUS = None


def corpus():
    """[(case, frame bytes, expected output)], built once per process."""
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = []
        for c in cases():
            fb = c.fr.bytes()
            _CORPUS.append((c, fb, model_frame(fb)))
    return _CORPUS


def owner(A: Analysis, pos: int):
    """(block, sequence, 'literal' | 'match') that produces output byte `pos` of the frame."""
    for b, B in enumerate(A.P.blocks):
        if pos < B["out_off"] + B["out_len"]:
            if B["stored"]: return b, None, "stored"
            S = B["seqs"]
            j = pos - B["out_off"]
            i = int(np.searchsorted(S[:, 1], j, side="right")) - 1
            return b, i, "literal" if j < S[i, 1] + S[i, 2] else "match"
    return None, None, "behind the content"


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_deps.json")


def fixture():
    sha = lambda b: hashlib.sha256(b).hexdigest()
    return {c.name: dict(frame_sha256=sha(fb), out_sha256=sha(out)) for c, fb, out in corpus()}


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(dict(cases=fixture()), f, indent=0, sort_keys=True)
        f.write("\n")
    tot = sum(len(o) for _, _, o in corpus())
    print("%d cases, %d bytes decoded -> %s" % (len(corpus()), tot, FIXTURE), file=sys.stderr)
