"""Many small frames: the batch call (lz4f_mi355x_dev_decompressFrames) against a loop of single calls and against one frame
holding the same blocks.  GPU box.

    python tools/batch_frames.py [--cases c1,c2,..] [--data synth50,text] [--timeout S]

For every case and input, a child process (its own time limit) compresses the frames on the GPU and decodes them
  batch  one decompress_frames_async call for all frames
  loop   one dev_decompressFrame per frame (each reads its header back to the host)
  one    the same blocks as ONE frame through dev_decompressFrame, where the framing allows it
and measures them
  measure  (the case "measure" only, which skips loop and one) one measure_frames_async call for all frames - sizes and decode
           windows, nothing decoded - its records and offsets checked against the batch decode's
timed with torch events on the engine's stream (best of a few runs; the loop: one run), every output checked against the input.
Prints one JSON line per case and input: ms and GiB/s (of decoded bytes) for each way."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (frames, bytes per frame, blockSizeID, linked, one frame of the same blocks possible, window stride in the destination)
CASES = {
    "64k_x4096": (4096, 64 << 10, 4, False, True, 0),
    "4k_x65536": (65536, 4 << 10, 4, False, False, 0),     # (blocks shorter than the block size in the middle of a frame: not one frame of them)
    "1m_linked64k_x1024": (1024, 1 << 20, 4, True, True, 0),
    "4m_x256": (256, 4 << 20, 7, False, True, 0),
    "measure": (4096, 64 << 10, 4, False, False, 0),        # the measure call beside the batch decode (no loop, no single frame)
    "64k_x64_in_4g": (64, 64 << 10, 4, False, False, 64 << 20),   # a small batch into a big destination buffer (windows 64 MiB apart)
}


def child(case: str, data: str, runs: int) -> dict:
    import torch
    from lz4_frame_conduit_amd import conduit, datagen
    from lz4_frame_conduit_amd.device import Engine, synth50_device
    n, fb, bsid, linked, one_ok, stride = CASES[case]
    stride = stride or fb
    dev = "cuda:0"
    total = n * fb
    if data == "synth50":
        src = synth50_device(total, 5, dev)
    else:
        base = torch.from_numpy(datagen.synth_text(min(total, 64 << 20), 5)).to(dev)
        src = base.repeat((total + base.numel() - 1) // base.numel())[:total].contiguous()
    eng = Engine(0)
    L = eng.L
    p = conduit.make_preferences(blockSizeID=bsid, blockMode=0 if linked else 1)
    bound = eng.frame_bound(fb, p)
    slots = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    recs = eng.new_results(n)
    for i in range(n):                                           # (asynchronous: no host read in dev_compressFrame)
        r = L.lz4f_mi355x_dev_compressFrame(eng.h, ctypes.c_void_p(slots.data_ptr() + i * bound), bound, ctypes.c_void_p(src.data_ptr() + i * fb), fb,
                                            ctypes.byref(p), ctypes.c_void_p(recs.data_ptr() + 32 * i), None)
        assert not L.LZ4F_isError(r)
    made = eng.frame_results(recs)
    assert all(r.status == 0 for r in made)
    sizes = [r.size for r in made]
    so = [0]
    for s in sizes:
        so.append(so[-1] + s)
    frames = torch.cat([slots[i * bound:i * bound + sizes[i]] for i in range(n)])
    del slots
    so_t = torch.tensor(so, dtype=torch.int64, device=dev)
    do_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * stride
    do_t[n] = (n - 1) * stride + fb
    dst = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    windows = dst.view(n, stride)[:, :fb]

    def same():
        return torch.equal(windows, src.view(n, fb))
    out = {"case": case, "data": data, "frames": n, "frame_bytes": fb, "block_bytes": 1 << (8 + 2 * bsid), "linked": linked,
           "compressed_bytes": int(so[-1]), "decoded_bytes": total, "dst_bytes": dst.numel()}

    def timed(fn, k):
        best = None
        for _ in range(k):
            dst.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(eng.stream):
                a.record(eng.stream)
                fn()
                b.record(eng.stream)
            b.synchronize()
            ms = a.elapsed_time(b)
            best = ms if best is None else min(best, ms)
        return best

    def rate(ms):
        return {"ms": round(ms, 4), "GiB_s": round(total / ms / 1e-3 / (1 << 30), 2)}

    res = eng.new_results(n)
    timed(lambda: eng.decompress_frames_async(frames, so_t, dst, do_t, res), 1)            # (warm-up: the workspace)
    ms = timed(lambda: eng.decompress_frames_async(frames, so_t, dst, do_t, res), runs)
    rr = eng.frame_results(res)
    assert all(r.status == 0 and r.size == fb for r in rr) and all((r.flags >> 12) == 0x1000 for r in rr), "batch: a frame failed"
    assert same(), "batch: output differs"
    out["batch"] = rate(ms)

    if case == "measure":
        # the measure call on the same frames: every size, and windows the batch decoder takes as they are
        mres, moff = eng.new_results(n), torch.zeros(n + 1, dtype=torch.int64, device=dev)
        timed(lambda: eng.measure_frames_async(frames, so_t, mres, moff), 1)                   # (warm-up: the workspace)
        ms = timed(lambda: eng.measure_frames_async(frames, so_t, mres, moff), runs)
        mm = eng.frame_results(mres)
        assert all(m.status == 0 and (m.size, m.consumed, m.n_blocks, m.flags) == (r.size, r.consumed, r.n_blocks, r.flags) for m, r in zip(mm, rr)), "measure: a record differs"
        assert torch.equal(moff, torch.arange(0, n + 1, dtype=torch.int64, device=dev) * fb), "measure: windows differ from the sizes"
        out["measure"] = rate(ms)
        out["measure_over_batch"] = round(out["measure"]["ms"] / out["batch"]["ms"], 3)
        eng.close()
        return out

    def loop():
        for i in range(n):
            r = L.lz4f_mi355x_dev_decompressFrame(eng.h, ctypes.c_void_p(dst.data_ptr() + i * stride), fb, ctypes.c_void_p(frames.data_ptr() + so[i]),
                                                  sizes[i], ctypes.c_void_p(res.data_ptr() + 32 * i))
            assert not L.LZ4F_isError(r)
    ms = timed(loop, 1)
    rr = eng.frame_results(res)
    assert all(r.status == 0 and r.size == fb for r in rr) and same(), "loop: output differs"
    out["loop"] = dict(rate(ms), us_per_frame=round(ms * 1e3 / n, 2))

    if one_ok:
        # one frame of the same blocks: the first frame's header, every frame's blocks (header and EndMark cut off), one EndMark
        host = frames.cpu().numpy().tobytes()
        flg = host[4]
        hs = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
        body = b"".join(host[so[i] + hs:so[i + 1] - 4] for i in range(n))
        one = torch.frombuffer(bytearray(host[:hs] + body + b"\0\0\0\0"), dtype=torch.uint8).to(dev)
        timed(lambda: eng.decompress_frame_async(one, one.numel(), dst), 1)
        ms = timed(lambda: eng.decompress_frame_async(one, one.numel(), dst), runs)
        r = eng.result()
        assert r.size == total and torch.equal(dst, src), "one frame: output differs"
        out["one_frame"] = dict(rate(ms), path=hex(r.flags >> 12))
        out["batch_over_one_frame"] = round(out["batch"]["ms"] / out["one_frame"]["ms"], 2)
    out["loop_over_batch"] = round(out["loop"]["ms"] / out["batch"]["ms"], 1)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--data", default="synth50,text")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case and input (a child process each)")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1], a.runs)), flush=True)
        return 0
    rc = 0
    for data in a.data.split(","):
        for case in a.cases.split(","):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", case, data],
                                   capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"case": case, "data": data, "error": "timeout after %d s" % a.timeout}), flush=True)
                return 1                                          # (nothing more on the GPU after a run that did not end)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                print(json.dumps({"case": case, "data": data, "error": "exit %d" % p.returncode, "stderr": p.stderr[-1500:]}), flush=True)
                return 1                                          # (a failed run may have left the device in a bad state: stop)
            print(line[-1], flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
