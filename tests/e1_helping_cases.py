"""Inputs for pass E1's long-sequence helpings (tests/test_gpu_e1_helpings.py; their oracle side in test_e1_helping_cases_cpu.py).

E1's units are a 128-byte slice, a helping of eight slices where sequences are long, and a 64 KiB tile; a run's first tile decides
between sparse and dense at slice 32, so the code behind that decision starts with a run's second tile.  A workgroup takes
n_tiles / CUs tiles (engine.hip: encode_plan), one tile for every input here - RUN_ENV makes an engine whose workgroups take runs of
sixteen, which is how inputs of 64 MiB and more are run by themselves.
"""
import numpy as np

from lz4_frame_conduit_amd import datagen

KIB = 1 << 10
RUN_ENV = {"LZ4F_MI355X_E1_RUN": "16"}
# (name, oracle.mkprefs keywords): 64 KiB linked, 64 KiB independent, 4 MiB independent blocks
FRAMINGS = [("linked64k", dict(bsid=4, indep=0)), ("indep64k", dict(bsid=4, indep=1)), ("indep4m", dict(bsid=7, indep=1))]
# inputs that are one run from end to end: the frame stays under 1 % of them
RUN_CASES = ("one_byte", "period4", "period5")


def _synth50(n: int) -> bytes:
    return datagen.synth50((n + 1023) // 1024 * 1024, 1234)[:n].tobytes()


def _rows500(n: int, lead: int) -> bytes:
    """Rows of 500 bytes, even rows random, odd rows a copy of an even row up to 119 rows back (inside the 64 KiB window); the
    stream begins `lead` bytes into row 0, so no helping begins or ends on a row."""
    rng = np.random.default_rng(500)
    rows = (n + lead + 499) // 500 + 1
    rows += rows & 1
    a = rng.integers(0, 256, rows * 500, dtype=np.uint8).reshape(-1, 500)
    odd = np.arange(1, rows, 2)
    src = np.maximum(odd - (rng.integers(1, 60, odd.size) * 2 + 1), 0)
    src -= src % 2
    a[odd] = a[src]
    return a.reshape(-1)[lead:lead + n].tobytes()


def _period(n: int, unit: bytes) -> bytes:
    return (unit * (n // len(unit) + 1))[:n]


def _straddle() -> bytes:
    """192 KiB of random bytes; a 3 KiB copy lies across each of the two tile boundaries (half of it on either side), so the tile
    behind each boundary opens inside a match - the second one directly behind a tile that was searched as sparse."""
    a = np.random.default_rng(192).integers(0, 256, 192 * KIB, dtype=np.uint8)
    a[64 * KIB - 1536:64 * KIB + 1536] = a[20000:20000 + 3072]
    a[128 * KIB - 1536:128 * KIB + 1536] = a[90000:90000 + 3072]
    return a.tobytes()


def _text_s50_text() -> bytes:
    t = datagen.synth_text(256 * KIB, 99).tobytes()
    return t[:128 * KIB] + _synth50(256 * KIB) + t[128 * KIB:]


_BUILD = {
    "s50_256k": lambda: _synth50(256 * KIB),
    "s50_1m77": lambda: _synth50(1024 * KIB + 77),               # a short last helping, a short last tile, a claim past the end of a partial tile
    "rows500": lambda: _rows500(320 * KIB, 200),
    "one_byte": lambda: _period(256 * KIB, b"\x5a"),
    "period4": lambda: _period(256 * KIB, b"\x01\x02\x03\x04"),      # the run candidate at stride 4 ...
    "period5": lambda: _period(256 * KIB, b"\x01\x02\x03\x04\x05"),  # ... and 5
    "straddle": _straddle,
    "text_s50_text": _text_s50_text,                                 # sparse <-> dense between tiles of one run
    "s50_4k": lambda: _synth50(4 * KIB),                             # a run that never leaves the undecided mode
    "s50_70k": lambda: _synth50(70 * KIB),
}
NAMES = tuple(_BUILD)
_CACHE = {}


def data(name: str) -> bytes:
    if name not in _CACHE:
        _CACHE[name] = _BUILD[name]()
    return _CACHE[name]


_ORACLE = {}


def oracle_frame(name: str, framing: str) -> bytes:
    """liblz4's frame (the oracle's port) of an input in a framing; made once."""
    import oracle
    if (name, framing) not in _ORACLE:
        _ORACLE[(name, framing)] = oracle.conduit_compress(data(name), oracle.mkprefs(**dict(FRAMINGS)[framing]))
    return _ORACLE[(name, framing)]
