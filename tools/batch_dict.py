"""Many small records with a shared dictionary: the batch calls with and without `dictionary=`, and with a prepared one (`cdict=`).  GPU box.

    python tools/batch_dict.py [--cases c1,c2,..] [--runs N] [--timeout S] [--level L]

Cases
  plain_64k_x4096    the plain batch calls at the README's shape (synth50 and text, level 0): no dictionary anywhere, so the same
                     command on two commits compares the kernels the plain calls launch
  dict_1k_x16384     records of 1 KiB / 16 KiB stitched from 32-byte slices of a 64 KiB phrase dictionary with a random byte
  dict_16k_x4096     between them: compress and decode with the dictionary beside the plain calls on the same records, and the
                     plain frames decoded through the dictionary call (its independent blocks go through the scalar-parse
                     decoder, the plain call's through the lanes' decoder: the cost of that routing on text-like records).
                     Then the prepared dictionary: create_cdict timed alone (the copy and the digest kernel), and the three
                     compress calls - dictionary=, cdict=, plain - timed by turns in one loop ("alternating"), the cdict's frames
                     and records checked to be the dictionary call's, byte for byte
  dict1k_1k_x16384   the same records with the dictionary's last 1 KiB as the dictionary (d1k): there the digest's 11.25 KiB are
  dict1k_16k_x4096   more than the dictionary they stand for
--level L (3-12; the default 0 is everything above): the plain case runs at that level, and a dictionary case becomes the prepared
dictionary with the hash-chain digest (create_cdict(d, hc=True)): create_cdict timed with and without hc by turns, then three compress
calls by turns - the HC CDict at level L, the plain call at level L, the CDict at level 0 - each with its compressed bytes beside
its time, the HC CDict's frames decoded through the dictionary decoder and checked against the input.
Every case runs in a child process with its own time limit.  Timed with torch events on the engine's stream: a warm-up call, then
`runs` calls, each timed on its own - the minimum, the median and the spread ((max - min) / min) are reported; GiB/s are of
uncompressed bytes over the minimum.  Every output is checked against the input.  One JSON line per case."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {                       # name: (records, bytes per record, dictionary bytes: the phrase dictionary's last ones; 0: none)
    "plain_64k_x4096": (4096, 64 << 10, 0),
    "dict_1k_x16384": (16384, 1 << 10, 65525),
    "dict_16k_x4096": (4096, 16 << 10, 65525),
    "dict1k_1k_x16384": (16384, 1 << 10, 1024),
    "dict1k_16k_x4096": (4096, 16 << 10, 1024),
}
DICT_BYTES = 65525
PIECE = 32


def phrase_dictionary(np):
    r = np.random.Generator(np.random.PCG64(11))
    pool = [bytes(r.integers(97, 123, int(k), dtype=np.uint8)) for k in r.integers(5, 25, 900)]
    out = bytearray()
    while len(out) < DICT_BYTES:
        out += pool[int(r.integers(0, len(pool)))] + b" "
    return np.frombuffer(bytes(out[:DICT_BYTES]), dtype=np.uint8)


def stitched_records(np, d, n, fb):
    """n records of fb bytes: PIECE-byte slices of the dictionary, a random byte behind each."""
    r = np.random.Generator(np.random.PCG64(12))
    k = (fb + PIECE) // (PIECE + 1)
    starts = r.integers(0, len(d) - PIECE, (n, k))
    rec = np.empty((n, k, PIECE + 1), dtype=np.uint8)
    rec[:, :, :PIECE] = d[starts[:, :, None] + np.arange(PIECE)[None, None, :]]
    rec[:, :, PIECE] = r.integers(0, 256, (n, k), dtype=np.uint8)
    return np.ascontiguousarray(rec.reshape(n, -1)[:, :fb])


def child(case: str, runs: int, level: int = 0) -> "list[dict]":
    import numpy as np
    import torch
    from lz4_frame_conduit_amd import conduit, datagen
    from lz4_frame_conduit_amd.device import Engine, frame_windows, synth50_device
    n, fb, dict_bytes = CASES[case]
    dev, total = "cuda:0", n * fb
    eng = Engine(0)
    p = conduit.make_preferences(blockSizeID=4, blockMode=1, compressionLevel=level)
    p0 = conduit.make_preferences(blockSizeID=4, blockMode=1)
    so_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * fb
    bound = frame_windows([fb], p)[1]
    wo_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * bound
    slots = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    res = eng.new_results(n)

    def timed_by_turns(fns: dict) -> dict:
        """name -> timing; in every round each call runs once, in the given order, timed on its own"""
        ms = {name: [] for name in fns}
        for k in range(runs + 1):                                    # (the first: warm-up - the workspace, the code objects)
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(eng.stream):
                    a.record(eng.stream)
                    fn()
                    b.record(eng.stream)
                b.synchronize()
                if k: ms[name].append(a.elapsed_time(b))
        out = {}
        for name, v in ms.items():
            v.sort()
            out[name] = {"ms_min": round(v[0], 4), "ms_median": round(v[len(v) // 2], 4), "spread": round((v[-1] - v[0]) / v[0], 3),
                         "GiB_s": round(total / v[0] / 1e-3 / (1 << 30), 2)}
        return out

    def timed(fn):
        return timed_by_turns({"": fn})[""]

    def roundtrip(src, cdict, ddict, frames_from=None):
        """compress with cdict (or take frames_from = (frames, offsets)), decode with ddict -> (compress timing, decode timing, frames, offsets, bytes)"""
        enc = None
        if frames_from is None:
            kw = {"dictionary": cdict} if cdict is not None else {}
            enc = timed(lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p, res, **kw))
            made = eng.frame_results(res)
            assert all(r.status == 0 and r.consumed == fb for r in made), "compress: a frame failed"
            sizes = torch.tensor([r.size for r in made], dtype=torch.int64, device=dev)
            fo_t = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            fo_t[1:] = torch.cumsum(sizes, 0)
            keep = (torch.arange(bound, device=dev)[None, :] < sizes[:, None]).reshape(-1)
            frames = slots[keep].contiguous()
        else:
            frames, fo_t = frames_from
        kw = {"dictionary": ddict} if ddict is not None else {}
        back.zero_()
        dec = timed(lambda: eng.decompress_frames_async(frames, fo_t, back, so_t, res, **kw))
        rr = eng.frame_results(res)
        assert all(r.status == 0 and r.size == fb for r in rr) and torch.equal(back, src), "decode: output differs"
        return enc, dec, frames, fo_t, int(fo_t[-1])

    outs = []
    if not dict_bytes:
        for data in ("synth50", "text"):
            if data == "synth50": src = synth50_device(total, 5, dev)
            else:
                base = torch.from_numpy(datagen.synth_text(min(total, 64 << 20), 5)).to(dev)
                src = base.repeat((total + base.numel() - 1) // base.numel())[:total].contiguous()
            enc, dec, _, _, cbytes = roundtrip(src, None, None)
            outs.append({"case": case, "data": data, "level": level, "records": n, "record_bytes": fb, "compressed_bytes": cbytes, "compress": enc, "decompress": dec})
    elif level >= 3:
        d_np = phrase_dictionary(np)
        d = torch.from_numpy(d_np[-dict_bytes:].copy()).to(dev)
        src = torch.from_numpy(stitched_records(np, d_np, n, fb)).to(dev).reshape(-1)
        made = {"plain": [], "hc": []}
        create = timed_by_turns({"create_cdict": lambda: made["plain"].append(eng.create_cdict(d)),
                                 "create_cdict_hc": lambda: made["hc"].append(eng.create_cdict(d, hc=True))})
        for v in create.values(): del v["GiB_s"]
        for c in made["plain"][:-1] + made["hc"][:-1]: c.close()
        cd, cd_hc = made["plain"][-1], made["hc"][-1]

        def frames_bytes(pp, **kw):
            """one call -> the frames' bytes in all; every frame made"""
            slots.zero_(); res.zero_()
            eng.compress_frames_async(src, so_t, slots, wo_t, pp, res, **kw)
            rr = eng.frame_results(res)
            assert all(r.status == 0 and r.consumed == fb for r in rr), "compress: a frame failed"
            return sum(r.size for r in rr), rr

        c_plain, _ = frames_bytes(p)
        c_cd0, _ = frames_bytes(p0, cdict=cd)
        c_hc, rr = frames_bytes(p, cdict=cd_hc)
        # the HC CDict's frames through the dictionary decoder
        sizes = torch.tensor([r.size for r in rr], dtype=torch.int64, device=dev)
        fo_t = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        fo_t[1:] = torch.cumsum(sizes, 0)
        frames = slots[(torch.arange(bound, device=dev)[None, :] < sizes[:, None]).reshape(-1)].contiguous()
        back.zero_()
        eng.decompress_frames_async(frames, fo_t, back, so_t, res, dictionary=cd_hc)
        assert all(r.status == 0 and r.size == fb for r in eng.frame_results(res)) and torch.equal(back, src), "decode: output differs"
        turns = timed_by_turns({"hc_cdict": lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p, res, cdict=cd_hc),
                                "plain": lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p, res),
                                "cdict_level0": lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p0, res, cdict=cd)})
        turns["hc_cdict"]["compressed_bytes"], turns["plain"]["compressed_bytes"], turns["cdict_level0"]["compressed_bytes"] = c_hc, c_plain, c_cd0
        cd.close(); cd_hc.close()
        outs.append({"case": case, "data": "stitched", "level": level, "records": n, "record_bytes": fb, "dictionary_bytes": dict_bytes,
                     "create_by_turns": create, "compress_by_turns": turns})
    else:
        d_np = phrase_dictionary(np)
        d = torch.from_numpy(d_np[-dict_bytes:].copy()).to(dev)
        src = torch.from_numpy(stitched_records(np, d_np, n, fb)).to(dev).reshape(-1)
        enc0, dec0, frames0, fo0, c0 = roundtrip(src, None, None)
        enc1, dec1, _, _, c1 = roundtrip(src, d, d)
        _, dec2, _, _, _ = roundtrip(src, None, d, frames_from=(frames0, fo0))      # the plain frames through the dictionary call's decoders
        # the prepared dictionary: its creation alone (each round makes one; close() waits for the stream, outside the events)
        made = []
        create = timed(lambda: made.append(eng.create_cdict(d)))
        del create["GiB_s"]
        for c in made[:-1]: c.close()
        cd = made[-1]
        slots.zero_(); res.zero_()
        eng.compress_frames_async(src, so_t, slots, wo_t, p, res, dictionary=d)
        eng.stream.synchronize()
        want = (slots.clone(), res.clone())
        slots.zero_(); res.zero_()
        eng.compress_frames_async(src, so_t, slots, wo_t, p, res, cdict=cd)
        eng.stream.synchronize()
        assert torch.equal(res, want[1]) and torch.equal(slots, want[0]), "cdict: the frames are not the dictionary call's"
        turns = timed_by_turns({"dictionary": lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p, res, dictionary=d),
                                "cdict": lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p, res, cdict=cd),
                                "plain": lambda: eng.compress_frames_async(src, so_t, slots, wo_t, p, res)})
        cd.close()
        outs.append({"case": case, "data": "stitched", "records": n, "record_bytes": fb, "dictionary_bytes": dict_bytes,
                     "plain": {"compressed_bytes": c0, "compress": enc0, "decompress": dec0},
                     "dictionary": {"compressed_bytes": c1, "compress": enc1, "decompress": dec1},
                     "plain_frames_scalar_parse_decode": dec2,
                     "bytes_plain_over_dictionary": round(c0 / c1, 2),
                     "create_cdict": create, "compress_by_turns": turns})
    eng.close()
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case (a child process each)")
    ap.add_argument("--level", type=int, default=0, help="0 (levels 0-2: the cases as described) or 3-12 (the HC CDict)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.level != 0 and not 3 <= a.level <= 12:
        ap.error("--level must be 0 or 3-12")
    if a.child:
        for o in child(a.child, a.runs, a.level):
            print(json.dumps(o), flush=True)
        return 0
    for case in a.cases.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--level", str(a.level), "--child", case], capture_output=True, text=True, timeout=a.timeout)
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
