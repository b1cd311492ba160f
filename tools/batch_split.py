"""The frame boundaries of a concatenated LZ4 stream found on the device (Engine.split_frames_async), beside the serial walk on the
device, beside what a caller does without the call, and beside the floor of streaming the bytes once.  GPU box.

    python tools/batch_split.py [--cases c1,c2,..] [--runs N] [--timeout S]

Cases (each: the inputs compressed by compress_frames_async and packed by pack_frames_async without a directory - the stream)
  dict_1k_x16384             16 384 records of 1 KiB stitched from a 64 KiB phrase dictionary, through a CDict: frames of about 350 bytes
  synth50_64k_x4096          4096 inputs of 64 KiB, synth50
  synth50_32m_x8             8 inputs of 32 MiB, synth50, in 64 KiB blocks: 512 blocks a frame
  synth50_64k_x4096_wrapped  the second stream with every frame wrapped in a stored block of an outer frame (4 MiB block size): an archive
                             of .lz4 files - 4096 true frames and 4096 false candidates
Variants, timed by turns in one loop (in every round each runs once, in this order, timed on its own)
  split          split_frames_async
  split_serial   the same on an engine made with LZ4F_MI355X_SPLIT_SERIAL: one thread walks
  today          a device-to-host copy of the stream (into page-locked memory), lz4f_mi355x_splitFrames - the same walk by the library's
                 grammar on one host thread - and the upload of the offsets
  copy           one contiguous device-to-device copy_ of the stream's bytes: the streaming floor
Every case runs in a child process with its own time limit.  Timed with torch events on the engine's stream: a warm-up round, then
`runs` rounds - the minimum, the median and the spread ((max - min) / min); GiB/s are of stream bytes over the minimum.  Every answer
is checked: the three routes give the same offsets, which are the pack's own (for the wrapped stream: the outer frames'), and the
record says what was found.  One JSON line per case, with split / copy, split / today and split / split_serial (of the minima)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = {                       # name: (inputs, bytes per input, blockSizeID, through a CDict of the phrase dictionary, wrapped)
    "dict_1k_x16384": (16384, 1 << 10, 4, True, False),
    "synth50_64k_x4096": (4096, 64 << 10, 4, False, False),
    "synth50_32m_x8": (8, 32 << 20, 4, False, False),
    "synth50_64k_x4096_wrapped": (4096, 64 << 10, 4, False, True),
}
PATH_BATCH, PATH_PARALLEL_WALK = 0x1000, 0x004


def make_stream(eng, torch, np, case):
    """-> (the stream on the device, the offsets of its true frames and its length as a list)"""
    import batch_dict
    from lz4_frame_conduit_amd import conduit
    from lz4_frame_conduit_amd.device import frame_windows, synth50_device
    n, fb, bsid, with_dict, wrapped = CASES[case]
    dev = "cuda:0"
    p = conduit.make_preferences(blockSizeID=bsid, blockMode=1)
    so_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * fb
    bound = frame_windows([fb], p)[1]
    wo_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * bound
    slots = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    res = eng.new_results(n)
    if with_dict:
        d_np = batch_dict.phrase_dictionary(np)
        cd = eng.create_cdict(torch.from_numpy(d_np.copy()).to(dev))
        src = torch.from_numpy(batch_dict.stitched_records(np, d_np, n, fb)).to(dev).reshape(-1)
        eng.compress_frames_async(src, so_t, slots, wo_t, p, res, cdict=cd)
    else:
        src = synth50_device(n * fb, 5, dev)
        eng.compress_frames_async(src, so_t, slots, wo_t, p, res)
    made = eng.frame_results(res)
    assert all(r.status == 0 and r.consumed == fb for r in made), "compress: a frame failed"
    packed = torch.zeros(sum(r.size for r in made), dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    eng.pack_frames_async(slots, wo_t, res, packed, off)
    eng.stream.synchronize()
    starts = off.cpu().tolist()
    if with_dict:
        cd.close()
    if not wrapped:
        return packed, starts
    import oracle
    head = oracle.header_bytes(oracle.mkprefs(bsid=7, indep=1))               # 7 bytes; the frame inside is one stored block
    host, out, at = packed.cpu().numpy().tobytes(), bytearray(), []
    for i in range(n):
        inner = host[starts[i]:starts[i + 1]]
        at.append(len(out))
        out += head + (0x80000000 | len(inner)).to_bytes(4, "little") + inner + bytes(4)
    at.append(len(out))
    return torch.from_numpy(np.frombuffer(bytes(out), dtype=np.uint8).copy()).to(dev), at


def child(case: str, runs: int) -> dict:
    import numpy as np
    import torch
    from lz4_frame_conduit_amd._ffi import Result
    from lz4_frame_conduit_amd.device import Engine
    n = CASES[case][0]
    dev = "cuda:0"
    eng = Engine(0)
    os.environ["LZ4F_MI355X_SPLIT_SERIAL"] = "1"
    ser = Engine(0)
    del os.environ["LZ4F_MI355X_SPLIT_SERIAL"]
    stream, starts = make_stream(eng, torch, np, case)
    size = stream.numel()
    off = {k: torch.full((n + 1,), -1, dtype=torch.int64, device=dev) for k in ("split", "split_serial", "today")}
    rec = {k: eng.new_results(1) for k in ("split", "split_serial")}
    pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
    h_off = torch.empty(n + 1, dtype=torch.int64).pin_memory()
    h_rec = Result()
    floor = torch.empty_like(stream)
    L = eng.L

    def today():
        with torch.cuda.stream(eng.stream):
            pinned.copy_(stream, non_blocking=True)
        eng.stream.synchronize()                                              # the synchronisation the device call is there to avoid
        r = L.lz4f_mi355x_splitFrames(pinned.data_ptr(), size, n, h_off.data_ptr(), ctypes.byref(h_rec))
        assert r == 0
        with torch.cuda.stream(eng.stream):
            off["today"].copy_(h_off, non_blocking=True)

    fns = {"split": lambda: eng.split_frames_async(stream, n, off["split"], record=rec["split"]),
           "split_serial": lambda: ser.split_frames_async(stream, n, off["split_serial"], record=rec["split_serial"]),
           "today": today,
           "copy": lambda: floor.copy_(stream, non_blocking=True)}
    ms = {name: [] for name in fns}
    for k in range(runs + 1):                                                 # (the first: warm-up - the workspace, the code objects)
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(eng.stream):
                a.record(eng.stream)
                fn()
                b.record(eng.stream)
            b.synchronize()
            if k: ms[name].append(a.elapsed_time(b))
    timing = {}
    for name, v in ms.items():
        v.sort()
        timing[name] = {"ms_min": round(v[0], 4), "ms_median": round(v[len(v) // 2], 4), "spread": round((v[-1] - v[0]) / v[0], 3),
                        "GiB_s": round(size / v[0] / 1e-3 / (1 << 30), 2)}
    # ---- every answer ----
    eng.stream.synchronize()
    want = torch.tensor(starts, dtype=torch.int64, device=dev)
    for k in off:
        assert torch.equal(off[k], want), "%s: not the frames' offsets" % k
    inner = sum(b - a for a, b in zip(starts, starts[1:]))
    for k, path in (("split", PATH_BATCH | PATH_PARALLEL_WALK), ("split_serial", PATH_BATCH)):
        r = eng.frame_results(rec[k])[0]
        assert (r.status, r.consumed, r.n_blocks, r.size, r.first_bad_block, r.flags >> 12) == (0, size, n, inner, 0xFFFFFFFF, path), (k, r.status, r.n_blocks, hex(r.flags))
    assert (h_rec.status, h_rec.consumed, h_rec.n_blocks) == (0, size, n), "today: the record"
    assert torch.equal(floor, stream)
    ser.close()
    eng.close()
    return {"case": case, "frames": n, "stream_bytes": size, **timing,
            "split_over_copy": round(timing["split"]["ms_min"] / timing["copy"]["ms_min"], 2),
            "split_over_today": round(timing["split"]["ms_min"] / timing["today"]["ms_min"], 4),
            "split_over_split_serial": round(timing["split"]["ms_min"] / timing["split_serial"]["ms_min"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case (a child process each)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.runs)), flush=True)
        return 0
    for case in a.cases.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", case], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": case, "error": "timeout after %d s" % a.timeout}), flush=True)
            return 1                                              # (nothing more on the GPU after a run that did not end)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print(json.dumps({"case": case, "error": "exit %d" % p.returncode, "stderr": p.stderr[-1500:]}), flush=True)
            return 1                                              # (a failed run may have left the device in a bad state: stop)
        for ln in lines:
            print(ln, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
