"""The dictionary encoders of the batch call on the planted corpus of dict_encoder_cases.py: the reach edge (a source exactly 65535
back, and 65536), the seam (a match's source lies on one side of it), dictionaries of 4 and 7 bytes, the dictionary in front of
every block of an independent frame and of a linked frame's first 64 KiB only, and a match at a frame's first byte.

Encoders:  U0   lz4f_mi355x_dev_compressFrames_usingDict, level 0 (k_bc_find_solo<true, false>)
           P0, P2   ..._usingCDict with the plain CDict, levels 0 and 2 (k_bc_find_solo<true, true>)
           H3, H9, H12   ..._usingCDict with create_cdict(d, hc=True) (k_bc_find_hc<true>)
Framings:  i64, l64, l256 of encoder_cases.FRAMINGS.  One batch call per (encoder, framing, dictionary) carries all of that
dictionary's cases; it is made once and shared by the tests below (`runs`).

What the parse is held to: tests/golden/dict_planted.json has what liblz4 1.9.3 writes of every case at levels 0 and 9.  A (case,
framing) is forced where liblz4's chain search wrote the planted parse - the hash-chain levels must write it too.  The fast finders
(a table of one entry per slot) are held to it where the dictionary lies wholly in the densely seeded last KiB; of a 64 KiB
dictionary's plants at the reach edge liblz4's own fast finder finds none, so there the claim is the conditional one of
test_fast_finders_at_the_reach_edge.  Sizes against liblz4's are printed, not asserted: the parse is the assertion.
"""
import pytest

import dict_cases as dc
import dict_encoder_cases as de
import encoder_cases as ec
import lz4_writer_rules as wr
from lz4_frame_conduit_amd import conduit
from lz4_frame_conduit_amd.device import Engine
from test_gpu_cdict_batch import Encoded, decoded, dev_bytes

pytestmark = pytest.mark.gpu
ENCODERS = ("U0", "P0", "P2", "H3", "H9", "H12")
LEVEL = {"U0": 0, "P0": 0, "P2": 2, "H3": 3, "H9": 9, "H12": 12}
FAST, CHAIN = ("U0", "P0", "P2"), ("H3", "H9", "H12")
DICTS = tuple(de.DICT_LEN)

# Forced pairs an encoder does not parse as planted, by case (all its framings), each with the reason from its finder's code.  At
# most 1 in 16 of the pairs the encoder is held to, none from reach/* or seam/cross (test_exemptions_are_few_and_reasoned).
_ONE_ENTRY = ("the deterministic finder's table holds one position per slot and a later insert replaces an earlier one (encode_solo.cuh, "
              "probe A: `table[hA] = (uint16_t)pA`): when the probe reaches S, the slot of S's first bytes holds the input's own 8-byte "
              "copy of them, not the dictionary's position, so it writes 8 bytes from the input and the other 52 from the dictionary - "
              "as liblz4's fast finder does (the fixture's level-0 parse); choosing the longer of two sources takes a chain")
EXEMPT = {"U0": {"pick/k1k": _ONE_ENTRY}, "P0": {"pick/k1k": _ONE_ENTRY}, "P2": {"pick/k1k": _ONE_ENTRY}, "H3": {}, "H9": {}, "H12": {}}

# the families no pair of which a fast finder is held to the planted parse on: reach/far has 64 KiB dictionaries only (its rule is
# test_fast_finders_at_the_reach_edge's), pick is about choosing among two sources (EXEMPT: held to liblz4's fast parse instead)
FAST_NOT_HELD = {"reach/far", "pick"}

_RUNS, _STATE = {}, {}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    _RUNS.clear(); _STATE.clear()
    yield e
    _RUNS.clear(); _STATE.clear()
    e.close()


@pytest.fixture(scope="module")
def fx():
    f = de.load_fixture()
    de.check_sha(f)
    return f


def prefs(fr: str, level: int):
    f = ec.FRAMINGS[fr]
    return conduit.make_preferences(blockSizeID=f["bsid"], blockMode=0 if f["linked"] else 1, blockChecksum=int(f["bck"]),
                                    contentChecksum=int(f["cck"]), compressionLevel=level)


def how(eng, enc: str, dname: str) -> dict:
    """The dictionary argument of an encoder's call: the tensor, the plain CDict or the hash-chain one - made once per dictionary."""
    if dname not in _STATE:
        d = dev_bytes(de.dictionary(dname))
        _STATE[dname] = dict(dictionary=d, plain=eng.create_cdict(d), hc=eng.create_cdict(d, hc=True))
    s = _STATE[dname]
    return dict(dictionary=s["dictionary"]) if enc == "U0" else dict(cdict=s["plain"] if enc in FAST else s["hc"])


def encode(eng, enc: str, fr: str, dname: str, cases=None) -> Encoded:
    cases = de.of_dictionary(dname, fr) if cases is None else cases
    return Encoded(eng, [c.data for c in cases], prefs(fr, LEVEL[enc]), **how(eng, enc, dname))


def runs(eng, enc: str, fr: str, dname: str) -> dict:
    """case name -> what its frame showed, for one batch call: status, size against the bound, the audit's violations, the round
    trips, the sequences that straddle the seam, whether a ghost's byte lies in a match, both parses, the record and the bytes."""
    key = (enc, fr, dname)
    if key in _RUNS: return _RUNS[key]
    cases = de.of_dictionary(dname, fr)
    p = prefs(fr, LEVEL[enc])
    got = encode(eng, enc, fr, dname, cases)
    d = de.dictionary(dname)
    arg = how(eng, enc, dname)
    frames = [got.frame(i) for i in range(len(cases))]
    dec = decoded(eng, frames, [max(len(c.data), 1) for c in cases], arg.get("dictionary", arg.get("cdict")))
    out = {"": dict(untouched=got.untouched_behind(), all=got.all())}
    for i, c in enumerate(cases):
        data, frame, n, bs = c.data, frames[i], len(c.data), ec.BS[fr]
        rec = dict(status=got.recs[i].status, consumed=got.recs[i].consumed, size=len(frame), bound=eng.frame_bound(n, p), one=got.all()[i])
        rec["audit"] = wr.audit(frame, data, ec.FRAMINGS[fr], dict_len=c.D) if rec["status"] == 0 else ["status %d" % rec["status"]]
        v = dc.model_decode(frame, d) if rec["status"] == 0 else None
        rec["model"] = "" if v and v.ok and v.out == data and v.consumed == len(frame) else "the model: %s" % (v.why if v else "no frame")
        rec["device"] = "" if dec[i][0] == 0 and dec[i][1] == n and dec[i][6][:n] == data else "the device's decoder: status %d, %d bytes" % (dec[i][0], dec[i][1])
        seqs = de.frame_seqs(frame) if not rec["audit"] else None
        rec["seqs"] = seqs
        if seqs is not None:
            rec["straddlers"] = de.straddlers(seqs, n, bs, ec.FRAMINGS[fr]["linked"])
            rec["ghost_used"] = not de.literal_everywhere(seqs, n, bs, c.ghosts(fr))
            rec["parse"] = de.parse_of(c, fr, seqs)
            rec["raw"] = de.rows(seqs, n, bs, False)
        out[c.name] = rec
    _RUNS[key] = out
    return out


def held(enc: str, c) -> bool:
    """The pairs an encoder is held to the planted parse on (where forced): every one for the chain search; for the fast finders
    the dictionaries that lie wholly in the densely seeded last KiB - and reach/ghost of any dictionary: its parse is no match at
    all, and the background holds no other repeat for any finder."""
    return enc in CHAIN or c.D <= de.DENSE or c.fam == "reach/ghost"


def compared(eng, fx, enc: str, fr: str, dname: str):
    """-> (the forced pairs compared, by family; {case: (got, want)} where the parse is not the planted one)"""
    R = runs(eng, enc, fr, dname)
    seen, missed = {}, {}
    for c in de.of_dictionary(dname, fr):
        if not held(enc, c) or not de.is_forced(fx, c, fr) or c.name in EXEMPT[enc]: continue
        seen[c.fam] = seen.get(c.fam, 0) + 1
        want = c.expected(fr)
        if R[c.name].get("parse") != want: missed[c.name] = (R[c.name].get("parse"), want)
    return seen, missed


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fr", de.FRAMINGS)
@pytest.mark.parametrize("enc", ENCODERS)
def test_frames_keep_the_rules_the_seam_and_the_reach(eng, enc, fr):
    """Claims 1 and 2, every encoder, every case: status 0; no writer rule broken with the dictionary's bytes counted into the reach;
    the dictionary model and the device's dictionary decoder give the input back; the frame is within frame_bound and nothing is
    written behind it; every byte of every ghost is a literal; no sequence's source holds a dictionary byte and an input byte."""
    n = 0
    for dname in DICTS:
        R = runs(eng, enc, fr, dname)
        assert R[""]["untouched"], (dname, "bytes behind `size` were written")
        for name, r in R.items():
            if not name: continue
            what = (enc, fr, name)
            assert r["status"] == 0 and r["audit"] == [], (what, r["status"], r["audit"])
            assert not r["model"] and not r["device"], (what, r["model"], r["device"])
            assert r["size"] <= r["bound"], (what, r["size"], r["bound"])
            assert not r["ghost_used"], (what, r["raw"])
            assert r["straddlers"] == [], (what, r["straddlers"])
            n += 1
    assert n == len([1 for c in de.corpus() if fr in c.framings])


@pytest.mark.parametrize("fr", de.FRAMINGS)
def test_the_plain_cdict_is_using_dict(eng, fr):
    """Claim 3: P0's frames and records are U0's, byte for byte."""
    for dname in DICTS:
        assert runs(eng, "P0", fr, dname)[""]["all"] == runs(eng, "U0", fr, dname)[""]["all"], dname


@pytest.mark.parametrize("enc", CHAIN)
def test_chain_levels_are_functions_of_their_input(eng, enc):
    """Claim 3: two runs agree in every framing, and a batch of one gives every case the frame it has among the others."""
    dname = "k64k"
    for fr in de.FRAMINGS:
        first = runs(eng, enc, fr, dname)[""]["all"]
        assert all(v[0] == 0 for v in first)
        assert encode(eng, enc, fr, dname).all() == first, fr
    first = runs(eng, enc, "l64", dname)
    for c in de.of_dictionary(dname, "l64"):
        assert encode(eng, enc, "l64", dname, [c]).all()[0] == first[c.name]["one"], c.name


@pytest.mark.parametrize("fr", de.FRAMINGS)
@pytest.mark.parametrize("enc", ENCODERS)
def test_parse_is_the_planted_one(eng, fx, enc, fr):
    """Claims 4 and 5: on every forced pair an encoder is held to (`held`) its parse is the planted one - sequence by sequence
    for seam/*, neighbours merged elsewhere - but for the cases EXEMPT names."""
    total, missed = 0, {}
    for dname in DICTS:
        seen, bad = compared(eng, fx, enc, fr, dname)
        total += sum(seen.values())
        missed.update(bad)
    for name in EXEMPT[enc]:                                  # an exempt case writes what its reason says: liblz4's level-0 parse
        c = next(c for c in de.corpus() if c.name == name)
        if fr in c.framings:
            got, fast = runs(eng, enc, fr, c.dname)[name].get("parse"), de.parse_of(c, fr, fx["cases"][name][fr]["seqs0"])
            assert got == fast != c.expected(fr), (enc, fr, name, got, fast)
    print("%s %s: %d forced pairs compared, %d not as planted" % (enc, fr, total, len(missed)))
    for n, v in missed.items(): print("   ", n, v)
    assert total >= 30 and not missed, (len(missed), dict(list(missed.items())[:4]))


@pytest.mark.parametrize("fr", de.FRAMINGS)
@pytest.mark.parametrize("enc", FAST)
def test_fast_finders_at_the_reach_edge(eng, enc, fr):
    """Claim 5, the 64 KiB dictionaries: of reach/far's 600-byte plants a fast finder may find less than all (liblz4's finds
    nothing there) - but a match that covers a byte of the plant has the plant's distance and does not start in front of it."""
    n = 0
    for dname in ("k64k-1", "k64k", "k70k"):
        R = runs(eng, enc, fr, dname)
        for c in de.of_dictionary(dname, fr):
            if c.fam != "reach/far": continue
            (x, M, dist), = c.plants()
            if M != 600: continue
            assert dist == 65535
            for pos, ml, off, _ in R[c.name]["raw"]:
                if pos < x + M and x < pos + ml: assert off == dist and pos >= x, (enc, fr, c.name, (pos, ml, off))
            print("%s %s %s: %s" % (enc, fr, c.name, R[c.name]["raw"]))
            n += 1
    assert n == 6


def test_exemptions_are_few_and_reasoned(fx):
    names = {c.name: c for c in de.corpus()}
    for enc in ENCODERS:
        mine = [(c, fr) for c, fr in de.pairs() if held(enc, c) and de.is_forced(fx, c, fr)]
        exempt = [(c, fr) for c, fr in mine if c.name in EXEMPT[enc]]
        assert len(exempt) * 16 <= len(mine), (enc, len(exempt), len(mine))
        for n, why in EXEMPT[enc].items():
            assert n in names and len(why) > 40 and "encode_" in why, (enc, n)
            assert not names[n].fam.startswith("reach/") and names[n].fam != "seam/cross", (enc, n)


def test_families_reached(eng, fx):
    """Claim 6, counted from the runs: per encoder and family at least one forced pair was compared with its planted parse (the
    fast finders: reach/far by test_fast_finders_at_the_reach_edge's rule).  An empty parametrisation fails here.  Also the sizes."""
    for enc in ENCODERS:
        seen = {}
        for fr in de.FRAMINGS:
            for dname in DICTS:
                for fam, k in compared(eng, fx, enc, fr, dname)[0].items(): seen[fam] = seen.get(fam, 0) + k
        print("%s: %d forced pairs compared: %s" % (enc, sum(seen.values()), sorted(seen.items())))
        want = set(de.FAMILIES) - (FAST_NOT_HELD if enc in FAST else set())
        assert want <= set(seen), (enc, sorted(want - set(seen)))
        size = sum(r["size"] for fr in de.FRAMINGS for dn in DICTS for n, r in runs(eng, enc, fr, dn).items() if n)
        l0, l9 = (sum(fx["cases"][c.name][fr]["size%d" % lv] for c, fr in de.pairs()) for lv in (0, 9))
        print("%s: %d bytes on the planted corpus; liblz4 level 0 %d, level 9 %d" % (enc, size, l0, l9))
