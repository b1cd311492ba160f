"""Many small inputs: the batch encode call (lz4f_mi355x_dev_compressFrames) against a loop of single deterministic calls and
against one deterministic frame holding the same blocks.  GPU box.

    python tools/batch_compress.py [--cases c1,c2,..] [--data synth50,text] [--levels 0,3] [--runs N] [--timeout S]

For every case, input and level, a child process (its own time limit) compresses the inputs on the GPU
  batch  one compress_frames_async call for all inputs
  loop   one dev_compressFrame per input on an engine in deterministic mode (asynchronous: no host read-back)
  one    the same bytes as ONE deterministic frame through dev_compressFrame, where the framing gives the same blocks
timed with torch events on the engine's stream around the enqueued work (after a warm-up, the median of the runs; the loop: the
median of up to three).  The batch's frames are decoded by the batch decoder and compared with the source, and a sample is compared
byte for byte with the loop's.  Prints one JSON line per case, input and level: ms and GiB/s (of input bytes) for each way."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (inputs, bytes per input, blockSizeID, linked, one frame of the same blocks possible)
CASES = {
    "64k_x4096": (4096, 64 << 10, 4, False, True),
    "4k_x65536": (65536, 4 << 10, 4, False, False),        # (blocks shorter than the block size in the middle of a frame: not one frame of them)
    "1m_linked64k_x1024": (1024, 1 << 20, 4, True, False),  # (one linked frame lets matches cross the inputs' boundaries: not the same blocks)
    "4m_x256": (256, 4 << 20, 7, False, True),
}


def child(case: str, data: str, level: int, runs: int) -> dict:
    import torch
    from lz4_frame_conduit_amd import conduit, datagen
    from lz4_frame_conduit_amd.device import Engine, frame_windows, synth50_device
    n, fb, bsid, linked, one_ok = CASES[case]
    dev = "cuda:0"
    total = n * fb
    if data == "synth50":
        src = synth50_device(total, 5, dev)
    else:
        base = torch.from_numpy(datagen.synth_text(min(total, 64 << 20), 5)).to(dev)
        src = base.repeat((total + base.numel() - 1) // base.numel())[:total].contiguous()
    eng = Engine(0)
    det = Engine(0)
    det.set_deterministic(True)
    L = eng.L
    p = conduit.make_preferences(blockSizeID=bsid, blockMode=0 if linked else 1, compressionLevel=level)
    do = frame_windows([fb] * n, p)
    bound = do[1]
    so_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * fb
    do_t = torch.tensor(do, dtype=torch.int64, device=dev)
    dst = torch.empty(do[-1], dtype=torch.uint8, device=dev)
    out = {"case": case, "data": data, "level": level, "frames": n, "input_bytes": fb, "block_bytes": 1 << (8 + 2 * bsid), "linked": linked,
           "total_bytes": total}

    def timed(e, fn, k):
        ms = []
        for _ in range(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(e.stream):
                a.record(e.stream)
                fn()
                b.record(e.stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    def rate(ms):
        return {"ms": round(ms, 4), "GiB_s": round(total / ms / 1e-3 / (1 << 30), 2)}

    res = eng.new_results(n)
    timed(eng, lambda: eng.compress_frames_async(src, so_t, dst, do_t, p, res), 1)            # (warm-up: the workspace)
    ms = timed(eng, lambda: eng.compress_frames_async(src, so_t, dst, do_t, p, res), runs)
    rr = eng.frame_results(res)
    assert all(r.status == 0 and r.consumed == fb and (r.flags >> 12) == 0x1000 for r in rr), "batch: a frame failed"
    out["batch"] = rate(ms)
    out["compressed_bytes"] = int(sum(r.size for r in rr))
    back = torch.zeros(total, dtype=torch.uint8, device=dev)
    res2 = eng.new_results(n)
    eng.decompress_frames_async(dst, do_t, back, so_t, res2)
    assert all(r.status == 0 and r.size == fb for r in eng.frame_results(res2)) and torch.equal(back, src), "batch: the frames do not decode to the inputs"
    del back

    slots = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    recs = det.new_results(n)

    def loop():
        for i in range(n):
            r = L.lz4f_mi355x_dev_compressFrame(det.h, ctypes.c_void_p(slots.data_ptr() + i * bound), bound, ctypes.c_void_p(src.data_ptr() + i * fb), fb,
                                                ctypes.byref(p), ctypes.c_void_p(recs.data_ptr() + 32 * i), None)
            assert not L.LZ4F_isError(r)
    timed(det, loop, 1)
    ms = timed(det, loop, min(runs, 3))
    made = det.frame_results(recs)
    for i in (0, 1, n // 2, n - 1):
        assert made[i].status == 0 and made[i].size == rr[i].size and torch.equal(slots[i * bound:i * bound + made[i].size], dst[do[i]:do[i] + rr[i].size]), \
            "frame %d differs between the batch and the single call" % i
    out["loop"] = dict(rate(ms), us_per_frame=round(ms * 1e3 / n, 2))
    del slots

    if one_ok:
        one = torch.empty(det.frame_bound(total, p), dtype=torch.uint8, device=dev)
        timed(det, lambda: det.compress_async(src, one, p), 1)
        ms = timed(det, lambda: det.compress_async(src, one, p), runs)
        r = det.result()
        assert r.n_blocks == total >> (8 + 2 * bsid)
        out["one_frame"] = rate(ms)
        out["batch_over_one_frame"] = round(out["batch"]["ms"] / out["one_frame"]["ms"], 2)
    out["loop_over_batch"] = round(out["loop"]["ms"] / out["batch"]["ms"], 1)
    eng.close()
    det.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--data", default="synth50,text")
    ap.add_argument("--levels", default="0,3")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case, input and level (a child process each)")
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child[0], a.child[1], int(a.child[2]), a.runs)), flush=True)
        return 0
    for level in a.levels.split(","):
        for data in a.data.split(","):
            for case in a.cases.split(","):
                tag = {"case": case, "data": data, "level": int(level)}
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", case, data, level],
                                       capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(json.dumps(dict(tag, error="timeout after %d s" % a.timeout)), flush=True)
                    return 1                                      # (nothing more on the GPU after a run that did not end)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not line:
                    print(json.dumps(dict(tag, error="exit %d" % p.returncode, stderr=p.stderr[-1500:])), flush=True)
                    return 1                                      # (a failed run may have left the device in a bad state: stop)
                print(line[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
