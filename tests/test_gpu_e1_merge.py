"""Pass E1's tile merge on the GPU, through the one-wave probe (k_e1_merge_probe, lz4f_mi355x_debug_e1_merge): every case of
tests/e1_merge_cases.py with the form before round 7 and with E1_V9.  The record list, rec_offs, ChunkInfo (nrec, first_lit, tail_lit,
body_size), the mode word and the no-room counter of the new form equal the old form's and the model's.  The pool's bump pointer is each
form's own - the records kept, or the records found (an upper bound, reserved before the walk) - so lists are compared, not addresses;
nothing else in the workspace is touched: the neighbouring chunks' words, the pool outside the reservation, the words behind the pool."""
import ctypes

import numpy as np
import pytest

import e1_merge_cases as mc
from lz4_frame_conduit_amd import _ffi

pytestmark = pytest.mark.gpu

GUARD = 64                                   # records behind the pool that nobody may write
FILL = 0xA5A5A5A5A5A5A5A5
FILL32 = 0xA5A5A5A5


@pytest.fixture(scope="module")
def tiles():
    return mc.cases()


@pytest.fixture(scope="module")
def probe():
    import torch
    L = _ffi.lib()
    assert hasattr(L, "lz4f_mi355x_debug_e1_merge"), "the library does not export the merge probe"
    dev = "cuda:0"
    head = mc.rec_pool_at(mc.N_CHUNKS)

    def as_dev(a, dt):
        return torch.from_numpy(a.view(dt)).to(dev)

    def run(t, form):
        """one merge of tile t -> dict of what it left (the fields of mc.model, and `clean`: nothing else was written)"""
        words = head + t.pool + GUARD
        recs = np.full(words, FILL, dtype=np.uint64)
        recs[0], recs[1] = t.bump0, 0
        info = np.full(mc.N_CHUNKS * 8, FILL32, dtype=np.uint32)
        d_end, d_n, d_lists = as_dev(t.s_end, np.int32), as_dev(t.s_n, np.uint8), as_dev(t.lists, np.int64)
        d_recs, d_info = as_dev(recs, np.int64), as_dev(info, np.int32)
        d_mode = torch.full((1,), 7, dtype=torch.int32, device=dev)
        rc = L.lz4f_mi355x_debug_e1_merge(form, d_end.data_ptr(), d_n.data_ptr(), d_lists.data_ptr(), mc.N_CHUNKS, t.pool, mc.CHUNK, t.ts, t.te, t.bend, t.nslice,
                                          d_info.data_ptr(), d_recs.data_ptr(), d_mode.data_ptr())
        assert rc == 0, (t.name, form, rc)
        recs2 = d_recs.cpu().numpy().view(np.uint64)
        info2 = d_info.cpu().numpy().view(np.uint32)
        offs = recs2[8:head].view(np.uint32)
        nrec = int(info2[mc.CHUNK * 8])
        base = int(offs[mc.CHUNK]) if offs[mc.CHUNK] != FILL32 else None
        out = dict(nrec=nrec, first_lit=int(info2[mc.CHUNK * 8 + 1]), tail_lit=int(info2[mc.CHUNK * 8 + 2]), body_size=int(info2[mc.CHUNK * 8 + 3]),
                   mode=int(d_mode.item()), bump=int(recs2[0]), noroom=int(recs2[1]), base=base)
        assert nrec == 0 or (base is not None and base + nrec <= t.pool), (t.name, form, base, nrec)
        out["recs"] = recs2[head + base: head + base + nrec].copy() if nrec else np.zeros(0, dtype=np.uint64)
        # untouched: control words 2..7, the other chunks' offsets and ChunkInfo, this chunk's carry_in / flags / out_off (pass S writes them),
        # the pool outside [bump0, the bump pointer) and the guard behind it
        pool = recs2[head:]
        lo, hi = min(t.bump0, t.pool), min(out["bump"], t.pool)
        others = np.delete(offs, mc.CHUNK)
        keep = np.ones(mc.N_CHUNKS * 8, dtype=bool)
        keep[mc.CHUNK * 8: mc.CHUNK * 8 + 4] = False
        out["clean"] = bool((recs2[2:8] == FILL).all() and (others == FILL32).all() and (info2[keep] == FILL32).all() and
                            (pool[:lo] == FILL).all() and (pool[hi:] == FILL).all())
        return out

    return run


def _same(got, want, name, who):
    for k in ("nrec", "first_lit", "tail_lit", "body_size", "mode", "noroom"):
        assert got[k] == want[k], (name, who, k, got[k], want[k])
    assert np.array_equal(got["recs"], want["recs"]), (name, who)


def test_both_forms_are_the_model_on_every_case(tiles, probe):
    for t in tiles:
        old, new = probe(t, 0), probe(t, 1)
        m_old, m_new = mc.model(t, "kept"), mc.model(t, "found")
        _same(old, m_old, t.name, "form before / model")
        _same(new, m_new, t.name, "E1_V9 / model")
        _same(new, old, t.name, "E1_V9 / form before")
        assert old["clean"] and new["clean"], (t.name, old["clean"], new["clean"])
        # each form's reservation: what the bump pointer is advanced by, and that a tile with room got its list where the pointer stood
        assert old["bump"] == m_old["bump"] and new["bump"] == m_new["bump"], (t.name, old["bump"], new["bump"], m_old["bump"], m_new["bump"])
        for got, m in ((old, m_old), (new, m_new)):
            if m["room"]:
                assert got["base"] == m["base"], (t.name, got["base"], m["base"])


def test_probe_refuses_arguments_out_of_range():
    L = _ffi.lib()
    f = L.lz4f_mi355x_debug_e1_merge
    one = ctypes.c_void_p(16)
    assert f(2, one, one, one, 3, 100, 1, 65536, 131072, 131072, 512, one, one, one) == 1          # no such form
    assert f(1, one, one, one, 3, 100, 3, 65536, 131072, 131072, 512, one, one, one) == 1          # chunk outside the workspace
    assert f(1, one, one, one, 3, 100, 1, 65536, 131072, 131072, 513, one, one, one) == 1          # more slices than a tile has
    assert f(1, one, one, one, 3, 100, 1, 65536, 131073, 131073, 512, one, one, one) == 1          # a tile longer than 64 KiB
    assert f(1, one, one, one, 3, 100, 1, 65536, 131072, 131072, 511, one, one, one) == 1          # slices that do not cover the tile
    assert f(1, None, one, one, 3, 100, 1, 65536, 131072, 131072, 512, one, one, one) == 1
