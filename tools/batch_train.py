"""A dictionary trained from a batch of samples on the device (Engine.train_dict_async), alone, followed by create_cdict, and beside
what a caller does without the call.  GPU box.

    python tools/batch_train.py [--cases c1,c2,..] [--runs N] [--host-runs N] [--timeout S]

Cases (dictSize 64 KiB, the default parameters)
  uniform_1k_x2048     the 2048 training records of tests/train_model.py's `uniform` corpus (stitched from a phrase dictionary's tail)
  zipf_1k_x2048        the 2048 training records of its `zipf` corpus (20 000 phrases drawn with zipf(1.3))
  stitched_1k_x16384   16 384 records of 1 KiB stitched from a 64 KiB phrase dictionary (tools/batch_dict.py's records): 16 MiB of samples
Variants, timed by turns in one loop (in every round each runs once, in this order, timed on its own)
  train          train_dict_async
  train_cdict    train_dict_async and create_cdict behind it on the same stream (the CDict freed outside the timed span)
  host           the host route: the samples copied down into page-locked memory, a synchronisation, tests/train_model.py's numpy model
                 on one host thread, the dictionary uploaded - wall-clock, `--host-runs` rounds (it takes seconds); where the model
                 cannot be imported (a tree without tests/), the copies alone, and "model": false in the line
Every case runs in a child process with its own time limit.  The device variants are timed with torch events on the engine's stream:
a warm-up round, then `runs` rounds - the minimum, the median and the spread ((max - min) / min).  Every answer is checked: the
device's dictionary is the model's, byte for byte, and the record says what the model says.  One JSON line per case, with
train / host (of the minima)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = ("uniform_1k_x2048", "zipf_1k_x2048", "stitched_1k_x16384")
DICT = 65536


def samples(case: str, np, tm) -> bytes:
    if case == "stitched_1k_x16384":
        import batch_dict
        return batch_dict.stitched_records(np, batch_dict.phrase_dictionary(np), 16384, 1024).tobytes()
    return b"".join(tm.records(case.split("_")[0])[0])


def child(case: str, runs: int, host_runs: int) -> dict:
    import numpy as np
    import torch
    from lz4_frame_conduit_amd._ffi import Result
    from lz4_frame_conduit_amd.device import Engine
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import train_model as tm
    except ImportError:
        tm = None
    if tm is None and case != "stitched_1k_x16384":
        return {"case": case, "error": "tests/train_model.py builds this corpus"}
    dev = "cuda:0"
    eng = Engine(0)
    data = samples(case, np, tm)
    n = len(data) // 1024
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * 1024
    d = {k: torch.zeros(DICT, dtype=torch.uint8, device=dev) for k in ("train", "train_cdict", "host")}
    rec = eng.new_results(1)
    pinned = torch.empty(len(data), dtype=torch.uint8).pin_memory()
    h_dict = torch.zeros(DICT, dtype=torch.uint8).pin_memory()
    made = []

    def train_cdict():
        eng.train_dict_async(src, off, d["train_cdict"])
        made.append(eng.create_cdict(d["train_cdict"]))

    fns = {"train": lambda: eng.train_dict_async(src, off, d["train"], record=rec), "train_cdict": train_cdict}
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
            while made: made.pop().close()
    want = None
    ms["host"] = []
    for k in range(host_runs):
        t0 = time.perf_counter()
        with torch.cuda.stream(eng.stream):
            pinned.copy_(src, non_blocking=True)
        eng.stream.synchronize()                                              # the synchronisation the device call is there to avoid
        if tm is not None:
            want = tm.train(pinned.numpy().tobytes(), DICT)
            h_dict.copy_(torch.from_numpy(np.frombuffer(want.dict, dtype=np.uint8).copy()))
        with torch.cuda.stream(eng.stream):
            d["host"].copy_(h_dict, non_blocking=True)
        eng.stream.synchronize()
        ms["host"].append((time.perf_counter() - t0) * 1e3)
    timing = {}
    for name, v in ms.items():
        v.sort()
        timing[name] = {"ms_min": round(v[0], 4), "ms_median": round(v[len(v) // 2], 4), "spread": round((v[-1] - v[0]) / v[0], 3)}
    # ---- every answer ----
    eng.stream.synchronize()
    r = Result.from_buffer_copy(rec.cpu().numpy().tobytes())
    assert torch.equal(d["train"], d["train_cdict"]), "two calls, two dictionaries"
    if want is not None:
        assert torch.equal(d["train"], d["host"]), "the device's dictionary is not the model's"
        assert (r.size, r.consumed, r.n_blocks, r.status, r.flags & 0xFF) == (want.used, want.consumed, want.n_segments, 0, want.rounds_run), "the record"
    eng.close()
    return {"case": case, "samples": n, "sample_bytes": len(data), "dict_bytes": DICT, "used": r.size, "segments": r.n_blocks, "rounds": r.flags & 0xFF,
            "model": tm is not None, **timing, "train_over_host": round(timing["train"]["ms_min"] / timing["host"]["ms_min"], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case (a child process each)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.runs, a.host_runs)), flush=True)
        return 0
    for case in a.cases.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--host-runs", str(a.host_runs), "--child", case],
                               capture_output=True, text=True, timeout=a.timeout)
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
