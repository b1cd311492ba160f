"""A batch's frames packed into one contiguous stream on the device (Engine.pack_frames_async), beside the bound of a copy and beside
what a caller did before there was such a call.  GPU box.

    python tools/batch_pack.py [--cases c1,c2,..] [--runs N] [--timeout S]

Cases
  dict_1k_x16384     16 384 records of 1 KiB stitched from a 64 KiB phrase dictionary (tools/batch_dict.py's), compressed through a CDict
  synth50_64k_x4096  4096 inputs of 64 KiB, synth50
  synth50_32m_x8     8 inputs of 32 MiB, synth50, in 4 MiB blocks
Variants, timed by turns in one loop (in every round each runs once, in this order, timed on its own)
  pack               pack_frames_async
  pack_directory     the same with the frame directory in front
  copy               one contiguous device-to-device copy_ of as many bytes as the pack writes: the bound of a copy
  today              frame_results (a synchronisation and a read-back), a prefix sum on the host, one copy_ per frame
Every case runs in a child process with its own time limit.  Timed with torch events on the engine's stream: a warm-up round, then
`runs` rounds - the minimum, the median and the spread ((max - min) / min); GiB/s are of packed bytes over the minimum.  Every output
is checked: the pack's bytes and offsets are today's, the directory read back on the device gives the pack's offsets, and the packed
stream decodes to the inputs through the batch decoder.  One JSON line per case, with pack / copy and pack / today (of the minima)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = {                       # name: (inputs, bytes per input, blockSizeID, through a CDict of the phrase dictionary)
    "dict_1k_x16384": (16384, 1 << 10, 4, True),
    "synth50_64k_x4096": (4096, 64 << 10, 4, False),
    "synth50_32m_x8": (8, 32 << 20, 7, False),
}


def child(case: str, runs: int) -> dict:
    import numpy as np
    import torch
    import batch_dict
    from lz4_frame_conduit_amd import conduit
    from lz4_frame_conduit_amd.device import Engine, frame_windows, pack_directory_size, peek_pack_directory, synth50_device
    n, fb, bsid, with_dict = CASES[case]
    dev, total = "cuda:0", n * fb
    eng = Engine(0)
    p = conduit.make_preferences(blockSizeID=bsid, blockMode=1)
    so_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * fb
    bound = frame_windows([fb], p)[1]
    wo_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * bound
    slots = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    res = eng.new_results(n)
    cd = None
    if with_dict:
        d_np = batch_dict.phrase_dictionary(np)
        cd = eng.create_cdict(torch.from_numpy(d_np.copy()).to(dev))
        src = torch.from_numpy(batch_dict.stitched_records(np, d_np, n, fb)).to(dev).reshape(-1)
    else:
        src = synth50_device(total, 5, dev)
    eng.compress_frames_async(src, so_t, slots, wo_t, p, res, **({"cdict": cd} if cd is not None else {}))
    made = eng.frame_results(res)
    assert all(r.status == 0 and r.consumed == fb for r in made), "compress: a frame failed"
    D = pack_directory_size(n)
    packed = sum(r.size for r in made)
    out = {k: torch.zeros(D + packed + 64, dtype=torch.uint8, device=dev) for k in ("pack", "pack_directory", "copy", "today")}
    off = {k: torch.zeros(n + 1, dtype=torch.int64, device=dev) for k in ("pack", "pack_directory")}
    rec = eng.new_results(1)
    today_off = []

    def today():
        rr = eng.frame_results(res)                                   # the synchronisation the batch call was built to avoid
        o, dst, wins = [0], out["today"], bound
        for r in rr:
            o.append(o[-1] + r.size)
        with torch.cuda.stream(eng.stream):
            for i, r in enumerate(rr):
                dst[o[i]:o[i + 1]].copy_(slots[i * wins:i * wins + r.size], non_blocking=True)
        today_off[:] = o

    fns = {"pack": lambda: eng.pack_frames_async(slots, wo_t, res, out["pack"], off["pack"], record=rec),
           "pack_directory": lambda: eng.pack_frames_async(slots, wo_t, res, out["pack_directory"], off["pack_directory"], directory=True, record=rec),
           "copy": lambda: out["copy"][:packed].copy_(slots[:packed], non_blocking=True),
           "today": today}
    ms = {name: [] for name in fns}
    for k in range(runs + 1):                                        # (the first: warm-up - the workspace, the code objects)
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
                        "GiB_s": round(packed / v[0] / 1e-3 / (1 << 30), 2)}
    # ---- every output ----
    eng.stream.synchronize()
    want_off = torch.tensor(today_off, dtype=torch.int64, device=dev)
    assert torch.equal(off["pack"], want_off) and torch.equal(out["pack"][:packed], out["today"][:packed]), "pack: not today's bytes"
    assert not out["pack"][packed:].any(), "pack: bytes behind the stream were written"
    assert torch.equal(off["pack_directory"], want_off + D) and torch.equal(out["pack_directory"][D:D + packed], out["today"][:packed]), "pack with directory: not today's bytes"
    assert not out["pack_directory"][D + packed:].any(), "pack with directory: bytes behind the stream were written"
    pr = eng.frame_results(rec)[0]
    assert (pr.status, pr.size, pr.consumed, pr.n_blocks) == (0, D + packed, packed, n), "pack: the record"
    stream = out["pack_directory"][:pr.size]
    dir_bytes, stored, fbytes = peek_pack_directory(stream[:24].cpu().numpy().tobytes())
    assert (dir_bytes, stored, fbytes) == (D, n, packed), "peek"
    src_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    eng.read_pack_directory_async(stream, stored, src_off, record=rec)
    assert eng.frame_results(rec)[0].status == 0 and torch.equal(src_off, off["pack_directory"]), "the directory read back"
    back = torch.zeros(total, dtype=torch.uint8, device=dev)
    eng.decompress_frames_async(stream, src_off, back, so_t, res, **({"dictionary": cd} if cd is not None else {}))
    assert all(r.status == 0 and r.size == fb for r in eng.frame_results(res)) and torch.equal(back, src), "decode: output differs"
    if cd is not None: cd.close()
    eng.close()
    return {"case": case, "inputs": n, "input_bytes": fb, "window_bytes": bound, "packed_bytes": packed, "directory_bytes": D, **timing,
            "pack_over_copy": round(timing["pack"]["ms_min"] / timing["copy"]["ms_min"], 2),
            "pack_directory_over_copy": round(timing["pack_directory"]["ms_min"] / timing["copy"]["ms_min"], 2),
            "pack_over_today": round(timing["pack"]["ms_min"] / timing["today"]["ms_min"], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--runs", type=int, default=7)
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
