"""The walks that GUESS a block table - parallel, seeded, trailer - on the cases of tests/walk_cases.py.

A guessed list of size-word positions may only become the block table if it is the chain the size words themselves form
(frame_dev.cuh: k_walk_link, k_walk_verdict); otherwise the serial walk behind it makes the table.  Either way the record and the
bytes must be the plain walk's (walk_cases.model_record, held to the oracle by tests/test_walk_cases_cpu.py), and which of the two
happened is reported: LZ4F_MI355X_PATH_WALK_DELIVERED.  Every case runs on an engine with the default switches and on one that
plans no guessing walk (LZ4F_MI355X_SERIAL_WALK and LZ4F_MI355X_NO_TRAILER: the first alone leaves the trailer's list in use);
the two must agree with the model and so with each other, nothing may be written behind the room, and the bit must be set where
the case's name is listed under must_deliver, clear under must_decline and on the second engine.  For a `free` case the bit only
goes into the printed line.  The seeded cases (192 MiB and one of 768 MiB) are made and compared on the device."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import walk_cases as wc
from lz4_frame_conduit_amd.device import Engine
from test_gpu_parity import PATH

pytestmark = pytest.mark.gpu
DEV, GUARD, PAT = "cuda:0", 4096, 0xA5
SERIAL_ENV = {"LZ4F_MI355X_SERIAL_WALK": "1", "LZ4F_MI355X_NO_TRAILER": "1"}


@pytest.fixture(scope="module")
def engines():
    """(the engine with the default switches, the engine that plans the serial walk only).  Switches are read when an engine is made."""
    assert not any(k in os.environ for k in SERIAL_ENV)
    eng = Engine(0)
    os.environ.update(SERIAL_ENV)
    try:
        serial = Engine(0)
    finally:
        for k in SERIAL_ENV: del os.environ[k]
    yield eng, serial
    eng.close(); serial.close()


def device_buffer(c) -> torch.Tensor:
    """The case's buffer in device memory: a seeded case is made there (payload from torch's generator, the operations planted
    from the host), the others are walk_cases.materialize's bytes."""
    if c.kind != "seeded":
        return torch.from_numpy(wc.materialize(c)).to(DEV)
    g = torch.Generator(device=DEV); g.manual_seed(zlib.crc32(c.name.encode()))
    t = torch.randint(1, 0x80, (c.cap,), dtype=torch.uint8, device=DEV, generator=g)
    for op in c.ops:
        if op[0] == "fill": t[op[1]:op[1] + op[2]] = op[3]
        else:
            assert op[0] == "bytes"
            t[op[1]:op[1] + len(op[2])] = torch.from_numpy(np.frombuffer(op[2], dtype=np.uint8).copy()).to(DEV)
    return t


def run(eng, frame, cap, dst, room):
    """-> (the record, or the error code the call itself returned)"""
    dst.fill_(PAT)
    r = eng.L.lz4f_mi355x_dev_decompressFrame(eng.h, ctypes.c_void_p(dst.data_ptr()), room, ctypes.c_void_p(frame.data_ptr()), cap, ctypes.c_void_p(eng._res.data_ptr()))
    if eng.L.LZ4F_isError(r):
        eng.stream.synchronize()
        return (1 << 64) - r
    return eng._result()


@pytest.mark.parametrize("name", wc.names())
def test_walk_case(engines, name):
    c = wc.case(name)
    frame = device_buffer(c)
    assert frame.numel() == c.cap and frame.data_ptr() % 16 == 0
    want = wc.model_record(lambda p, n: frame[p:p + n].cpu().numpy().tobytes(), c.cap, c.room, checks=c.kind != "seeded")
    assert c.kind != "seeded" or not (c.bck or c.cck)
    content = torch.cat([frame[p:p + n] for p, n in c.segs]) if want["status"] == 0 and c.segs and not want["flags"] & 0x100 else frame[:0]
    assert content.numel() == want["size"] or want["status"] != 0
    dst = torch.empty(c.room + GUARD, dtype=torch.uint8, device=DEV)
    seen = []
    for serial, eng in enumerate(engines):
        got = run(eng, frame, c.cap, dst, c.room)
        assert bool((dst[c.room:] == PAT).all()), (name, serial, "bytes behind the room were written")
        if want["host"]:
            assert got == want["status"], (name, serial, got)
            seen.append(("host", got))
            continue
        assert not isinstance(got, int), (name, serial, "the call returned error", got)
        path = int(got.flags) >> 12
        delivered = bool(path & PATH["walk_delivered"])
        rec = dict(status=got.status, size=got.size, consumed=got.consumed, n_blocks=got.n_blocks, first_bad_block=got.first_bad_block, flags=got.flags & 0x1FF)
        print("%-32s %-7s %s path %#06x %s" % (name, "serial" if serial else "default", c.expect, path, "DELIVERED" if delivered else "walked"))
        assert rec == {k: want[k] for k in rec}, (name, serial, rec, want)
        if want["status"] == 0:
            assert torch.equal(dst[:want["size"]], content), (name, serial, "output")
        planned = "serial" if serial else c.planned
        assert bool(path & PATH["parallel_walk"]) == (planned == "parallel"), (name, serial, hex(path))
        assert bool(path & PATH["trailer"]) == (planned == "trailer"), (name, serial, hex(path))
        assert not path & PATH["table"], (name, serial, hex(path))
        if serial or c.expect == "must_decline":
            assert not delivered, (name, serial, c.expect, hex(path))
        elif c.expect == "must_deliver":
            assert delivered, (name, serial, c.expect, hex(path))
        seen.append(rec)
    assert seen[0] == seen[1], (name, seen)
