"""Mixed batches for the dictionary-set calls (test helper, not a test module; numpy + the oracle only).

A set has a member per dictionary of tests/dict_cases.py and one empty member; a batch's frames name their members by slot.  Built
from dict_cases alone - its dictionaries, natural records and fixture frames (tests/golden/dict_frames.json holds liblz4's CDict
frames for all five dictionaries) - so nothing new is minted:
  - MEMBERS / IDS: the set.  The IDs are unsorted, one is 0 (its frames carry no dictID field), one has the high bit set;
  - compress_inputs(): the natural records of all five dictionaries in one batch, the phrase dictionary's records of several
    chunks and blocks among them; slot_cycle(): slots that go round all members and DICT_NONE;
  - crossing_records(): many short records for a finder grid smaller than the batch, so that a workgroup strides from a chunk of
    one member to a chunk of another: record i is a slice of the dictionary that the same workgroup's chunk before it had;
  - decode_cases(): the fixture's frames of all dictionaries and both block modes, the planted ones that liblz4 rejects included;
  - patch_dict_id(): a frame with another dictID, its header checksum sealed again.
"""
from __future__ import annotations

import numpy as np

import dict_cases as dc
import oracle

NONE = 0xFFFFFFFF                                   # LZ4F_MI355X_DICT_NONE
UNKNOWN = 0xFFFFFFFE                                # LZ4F_MI355X_DICT_UNKNOWN
PATH_BATCH, PATH_DICT_UNKNOWN = 0x1000, 0x4000
ST_GENERIC = 1

MEMBERS = ("phrase", "d1k", "d1", "big", "d3", None)            # None: the empty member
IDS = (7, 0, 0x80000001, 3, 0xFFFFFFFF, 12)
ABSENT_ID = 0x1234
assert len(set(IDS)) == len(IDS) == len(MEMBERS) and ABSENT_ID not in IDS and list(IDS) != sorted(IDS)


def slot_of(name) -> int:
    return MEMBERS.index(name)


def slot_cycle(n: int, shift: int = 0) -> "list[int]":
    """n slots that go round every member and DICT_NONE."""
    ring = list(range(len(MEMBERS))) + [NONE]
    return [ring[(i + shift) % len(ring)] for i in range(n)]


def member_bytes(slot: int) -> bytes:
    """The dictionary a slot stands for (DICT_NONE and the empty member: none)."""
    return b"" if slot == NONE or MEMBERS[slot] is None else dc.dictionary(MEMBERS[slot])


def member_id(slot: int, prefs_id: int) -> int:
    """The dictID in the header of a frame with this slot (DICT_NONE: the call's own)."""
    return prefs_id if slot == NONE else IDS[slot]


def compress_inputs() -> "list[tuple[str, bytes]]":
    """About 60 inputs: every dictionary's natural records - the phrase dictionary's SMALL lengths 0 .. 4096, `slice`, `tail` and the
    BIG records of 65 535 / 65 536 / 65 537 / 131 085 bytes (chunks behind a scope's first, several blocks), the others' FEW."""
    out = []
    for dname in ("phrase", "d1k", "d1", "big", "d3"):
        for name, x in dc.natural(dname):
            if dname == "phrase" and name.startswith("x"): continue                 # (the ratio test's extra records)
            out.append(("%s/%s" % (dname, name), x))
    assert 50 <= len(out) <= 70 and sorted(len(x) for _, x in out)[-4:] == list(dc.BIG)
    return out


CROSS_RING = ("phrase", "d1k", NONE, "d3")


def crossing_slots(n: int, *strides: int) -> "list[int]":
    """Slots that alternate between phrase, d1k, DICT_NONE and d3 - and move on by one with every `stride` frames, for each stride, so
    that frames i and i + stride (one workgroup's consecutive chunks when the finder's grid is `stride`) never have the same one."""
    ring = [NONE if m is NONE else slot_of(m) for m in CROSS_RING]
    out = [ring[(i + sum(i // s for s in strides)) % 4] for i in range(n)]
    for s in strides:
        assert all(out[i] != out[i + s] for i in range(n - s)), s
    return out


def crossing_records(n: int, slots, stride: int, lo: int = 64, hi: int = 200) -> "list[bytes]":
    """n records of lo..hi bytes: record i is a slice of the dictionary of the slot that frame i - stride has (the phrase
    dictionary where that one has no bytes to speak of), from in front of its last KiB where that is possible - what a digest
    carried over from that chunk would find matches in, and record i's own member mostly cannot."""
    r = dc.rng_of("crossing/%d/%d" % (n, stride))
    lens = r.integers(lo, hi + 1, n)
    out = []
    for i in range(n):
        prev = slots[i - stride] if i >= stride else slots[(i + 1) % n]
        d = member_bytes(prev)
        if len(d) < 4096: d = dc.dictionary("d1k" if prev == slot_of("d1k") else "phrase")
        d = dc.tail(d)
        k = int(lens[i])
        at = int(r.integers(0, max(1, len(d) - 1024 - k))) if len(d) > 2048 else int(r.integers(0, len(d) - k))
        out.append(d[at:at + k])
    return out


def decode_cases(fx: dict) -> "list[tuple[str, bytes, bytes | None, int]]":
    """(name, frame, expected output or None where liblz4 rejects the frame, slot): the fixture's frames of all five dictionaries
    and both block modes in one batch, every frame with the slot of the dictionary it was made for."""
    out = []
    for dname in dc.DICT_LEN:
        for mode in dc.MODES:
            for name, frame, exp, _ in dc.fixture_frames(fx, dname, mode):
                out.append(("%s/%s/%s" % (dname, mode, name), frame, exp, slot_of(dname)))
    assert sum(1 for c in out if c[2] is None) >= 6 and any("off_plus1" in c[0] for c in out) and any("through_block1_plus1" in c[0] for c in out)
    return out


def dict_id_at(frame: bytes) -> "int | None":
    """Where a frame's dictID field stands (None: it has none)."""
    flg = frame[4]
    return (6 + (8 if flg & 8 else 0)) if flg & 1 else None


def patch_dict_id(frame: bytes, dict_id: int) -> bytes:
    """The frame with `dict_id` in its dictID field and the header checksum sealed again."""
    at = dict_id_at(frame)
    assert at is not None
    b = bytearray(frame)
    b[at:at + 4] = int(dict_id).to_bytes(4, "little")
    b[at + 4] = (oracle.xxh32(bytes(b[4:at + 4])) >> 8) & 0xFF
    return bytes(b)


def slots_array(slots) -> np.ndarray:
    """Slots as the int32 array a device tensor is made of (the values are uint32)."""
    return np.asarray(list(slots), dtype=np.uint32).view(np.int32)
