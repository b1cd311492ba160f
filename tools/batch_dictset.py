"""A mixed batch with a set of dictionaries, one chosen per frame: the set calls beside what a caller does without them.  GPU box.

    python tools/batch_dictset.py [--cases c1,c2,..] [--dicts 1,4,64] [--levels 0,3] [--runs N] [--timeout S]

Cases
  set_1k_x16384     the README's stitched records (tools/batch_dict.py: 32-byte slices of a 64 KiB phrase dictionary with a random
  set_16k_x4096     byte between them) dealt round-robin over K phrase dictionaries of 64 KiB from different seeds, record i stitched
                    from dictionary i mod K.  Level 0 with plain CDicts, level 3 with hash-chain CDicts.
Legs, per case, K and level, timed by turns in one loop (each call timed on its own in every round):
  compress   set        compress_frames_async(dictset=, slots=): the mixed batch in one call
             one_cdict  compress_frames_async(cdict=) with dictionary 0 on the same records: the one-dictionary kernels (for K = 1 the
                        same work; for K > 1 most records then lean on a dictionary they were not stitched from)
             grouped    what a caller does without the set: K compress_frames_async(cdict=) calls over the records grouped by
                        dictionary beforehand (the grouping itself and the scatter back are not timed)
  decode     set        decompress_frames_async(dictset=, slots=None): by each header's dictID
             set_slots  the same with the slots given
             one_dict / grouped   decompress_frames_async(dictionary=) over the one-dictionary frames / K calls over the grouped frames
  resolve    resolve_dict_ids_async alone
The set's frames are checked to be the grouped calls' frames, byte for byte, and every decode against the input.  Every (case, K,
level) runs in a child process with its own time limit.  Timed with torch events on the engine's stream: one warm-up round, then
`runs` rounds; the minimum, the median and the spread ((max - min) / min) are reported.  One JSON line per (case, K, level)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"set_1k_x16384": (16384, 1 << 10), "set_16k_x4096": (4096, 16 << 10)}       # name: (records, bytes per record)
DICT_BYTES = 65525
PIECE = 32


def phrase_dictionary(np, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    pool = [bytes(r.integers(97, 123, int(k), dtype=np.uint8)) for k in r.integers(5, 25, 900)]
    out = bytearray()
    while len(out) < DICT_BYTES:
        out += pool[int(r.integers(0, len(pool)))] + b" "
    return np.frombuffer(bytes(out[:DICT_BYTES]), dtype=np.uint8)


def stitched_records(np, d, n, fb, seed):
    """n records of fb bytes: PIECE-byte slices of the dictionary, a random byte behind each."""
    r = np.random.Generator(np.random.PCG64(seed))
    k = (fb + PIECE) // (PIECE + 1)
    starts = r.integers(0, len(d) - PIECE, (n, k))
    rec = np.empty((n, k, PIECE + 1), dtype=np.uint8)
    rec[:, :, :PIECE] = d[starts[:, :, None] + np.arange(PIECE)[None, None, :]]
    rec[:, :, PIECE] = r.integers(0, 256, (n, k), dtype=np.uint8)
    return np.ascontiguousarray(rec.reshape(n, -1)[:, :fb])


def child(case: str, K: int, level: int, runs: int) -> dict:
    import numpy as np
    import torch
    from lz4_frame_conduit_amd import conduit
    from lz4_frame_conduit_amd.device import Engine, frame_windows
    n, fb = CASES[case]
    assert n % K == 0
    dev, total, per = "cuda:0", n * fb, n // K
    eng = Engine(0)
    hc = level >= 3
    p = conduit.make_preferences(blockSizeID=4, blockMode=1, compressionLevel=level, dictID=1)       # (dictionary k has the ID k + 1)
    bound = frame_windows([fb], p)[1]
    dicts_np = [phrase_dictionary(np, 100 + k) for k in range(K)]
    dicts = [torch.from_numpy(d.copy()).to(dev) for d in dicts_np]
    cds = [eng.create_cdict(d, hc=hc) for d in dicts]
    dset = eng.create_dictset(cds, [k + 1 for k in range(K)])
    # record i is stitched from dictionary i % K; `grouped` holds the same records with dictionary k's in rows [k * per, (k + 1) * per)
    by_dict = [stitched_records(np, dicts_np[k], per, fb, 200 + k) for k in range(K)]
    mixed_np = np.empty((n, fb), dtype=np.uint8)
    for k in range(K): mixed_np[k::K] = by_dict[k]
    mixed = torch.from_numpy(mixed_np).to(dev).reshape(-1)
    grouped = torch.from_numpy(np.concatenate(by_dict)).to(dev).reshape(-1)
    slot_t = (torch.arange(n, dtype=torch.int32, device=dev) % K).contiguous()
    so_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * fb
    wo_t = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * bound
    go_t = [(so_t[k * per:(k + 1) * per + 1].contiguous(), wo_t[k * per:(k + 1) * per + 1].contiguous()) for k in range(K)]
    win = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    res = eng.new_results(n)
    RB = eng.RESULT_BYTES
    res_k = [res[k * per * RB:(k + 1) * per * RB] for k in range(K)]

    def timed_by_turns(fns: dict) -> dict:
        ms = {name: [] for name in fns}
        for r in range(runs + 1):                                    # (the first: warm-up - the workspace, the code objects)
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(eng.stream):
                    a.record(eng.stream)
                    fn()
                    b.record(eng.stream)
                b.synchronize()
                if r: ms[name].append(a.elapsed_time(b))
        out = {}
        for name, v in ms.items():
            v.sort()
            out[name] = {"ms_min": round(v[0], 4), "ms_median": round(v[len(v) // 2], 4), "spread": round((v[-1] - v[0]) / v[0], 3),
                         "GiB_s": round(total / v[0] / 1e-3 / (1 << 30), 2)}
        return out

    def c_set(): eng.compress_frames_async(mixed, so_t, win, wo_t, p, res, dictset=dset, slots=slot_t)
    def c_one(): eng.compress_frames_async(mixed, so_t, win, wo_t, p, res, cdict=cds[0])

    def c_grouped():
        for k in range(K):
            pk = conduit.make_preferences(blockSizeID=4, blockMode=1, compressionLevel=level, dictID=k + 1)
            eng.compress_frames_async(grouped, go_t[k][0], win, go_t[k][1], pk, res_k[k], cdict=cds[k])

    def packed():
        """the frames just made in `win`, back to back -> (frames, offsets, bytes in all)"""
        rr = eng.frame_results(res)
        assert all(r.status == 0 and r.consumed == fb for r in rr), "compress: a frame failed"
        sizes = torch.tensor([r.size for r in rr], dtype=torch.int64, device=dev)
        fo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        fo[1:] = torch.cumsum(sizes, 0)
        return win[(torch.arange(bound, device=dev)[None, :] < sizes[:, None]).reshape(-1)].contiguous(), fo, int(fo[-1])

    # the set's frames are the grouped calls' frames (record k * per + j of `grouped` is record j * K + k of `mixed`)
    win.zero_(); c_grouped(); eng.stream.synchronize()
    g_win, g_res = win.clone().reshape(K, per, bound), res.clone().reshape(K, per, RB)
    g_frames, g_fo, g_bytes = packed()
    win.zero_(); c_set(); eng.stream.synchronize()
    assert torch.equal(win.reshape(per, K, bound).transpose(0, 1), g_win) and torch.equal(res.reshape(per, K, RB).transpose(0, 1), g_res), \
        "the set's frames are not the grouped calls' frames"
    s_frames, s_fo, s_bytes = packed()
    win.zero_(); c_one(); eng.stream.synchronize()
    o_frames, o_fo, o_bytes = packed()
    compress = timed_by_turns({"set": c_set, "one_cdict": c_one, "grouped": c_grouped})
    compress["set"]["compressed_bytes"], compress["one_cdict"]["compressed_bytes"], compress["grouped"]["compressed_bytes"] = s_bytes, o_bytes, g_bytes

    gfo_k = [(g_fo[k * per:(k + 1) * per + 1].contiguous()) for k in range(K)]
    def d_set(): eng.decompress_frames_async(s_frames, s_fo, back, so_t, res, dictset=dset)
    def d_slots(): eng.decompress_frames_async(s_frames, s_fo, back, so_t, res, dictset=dset, slots=slot_t)
    def d_one(): eng.decompress_frames_async(o_frames, o_fo, back, so_t, res, dictionary=cds[0])

    def d_grouped():
        for k in range(K): eng.decompress_frames_async(g_frames, gfo_k[k], back, go_t[k][0], res_k[k], dictionary=cds[k])

    for fn, want in ((d_set, mixed), (d_slots, mixed), (d_one, mixed), (d_grouped, grouped)):
        back.zero_(); fn()
        assert all(r.status == 0 and r.size == fb for r in eng.frame_results(res)) and torch.equal(back, want), "decode: output differs"
    decode = timed_by_turns({"set": d_set, "set_slots": d_slots, "one_dict": d_one, "grouped": d_grouped})
    got = torch.empty(n, dtype=torch.int32, device=dev)
    resolve = timed_by_turns({"resolve": lambda: eng.resolve_dict_ids_async(s_frames, s_fo, dset, got)})["resolve"]
    del resolve["GiB_s"]
    eng.stream.synchronize()
    assert torch.equal(got, slot_t), "resolve: the slots differ"
    eng.close()
    return {"case": case, "dicts": K, "level": level, "records": n, "record_bytes": fb, "compress_by_turns": compress, "decode_by_turns": decode,
            "resolve": resolve}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--dicts", default="1,4,64")
    ap.add_argument("--levels", default="0,3")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per (case, K, level): a child process each")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        case, K, level = a.child.split(":")
        print(json.dumps(child(case, int(K), int(level), a.runs)), flush=True)
        return 0
    for case in a.cases.split(","):
        for level in a.levels.split(","):
            for K in a.dicts.split(","):
                what = "%s:%s:%s" % (case, K, level)
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", what], capture_output=True, text=True,
                                       timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"case": what, "error": "timeout after %d s" % a.timeout}), flush=True)
                    return 1                                          # (nothing more on the GPU after a run that did not end)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not lines:
                    print(json.dumps({"case": what, "error": "exit %d" % p.returncode, "stderr": p.stderr[-1500:]}), flush=True)
                    return 1                                          # (a failed run may have left the device in a bad state: stop)
                for ln in lines:
                    print(ln, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
