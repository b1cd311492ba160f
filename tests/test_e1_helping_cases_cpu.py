"""The oracle's side of tests/test_gpu_e1_helpings.py: what that file expects of the GPU encoder holds for liblz4's own frames.
Every input round-trips through the oracle in every framing, and the inputs that are one run compress to under 1 % there too."""
import pytest

import oracle
import e1_helping_cases as hc


@pytest.mark.parametrize("framing", [f for f, _ in hc.FRAMINGS])
def test_oracle_roundtrip_and_run_bound(framing):
    for name in hc.NAMES:
        d = hc.data(name)
        frame = hc.oracle_frame(name, framing)
        out, used = oracle.decompress_frame(frame, cap=len(d) + 64)
        assert used == len(frame) and out == d, (name, framing)
        if name in hc.RUN_CASES:
            assert len(frame) * 100 < len(d), (name, framing, len(frame))


def test_inputs_are_what_the_cases_say():
    sizes = {n: len(hc.data(n)) for n in hc.NAMES}
    assert sizes == {"s50_256k": 256 << 10, "s50_1m77": (1 << 20) + 77, "rows500": 320 << 10, "one_byte": 256 << 10, "period4": 256 << 10,
                     "period5": 256 << 10, "straddle": 192 << 10, "text_s50_text": 512 << 10, "s50_4k": 4 << 10, "s50_70k": 70 << 10}
    s = hc.data("straddle")
    assert s[(64 << 10) - 1536:(64 << 10) + 1536] == s[20000:23072] and s[(128 << 10) - 1536:(128 << 10) + 1536] == s[90000:93072]
    p5 = hc.data("period5")
    assert p5[5:] == p5[:-5] and p5[4:] != p5[:-4]
    # rows of 500 bytes, 200 bytes into the first: rows begin at 300, 800, ... and row 1 is a copy of row 0, whose last 300 bytes the stream has
    r = hc.data("rows500")
    assert r[500:800] == r[0:300] and r[300:500] != r[800:1000]
