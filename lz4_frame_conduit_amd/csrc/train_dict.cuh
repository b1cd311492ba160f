// train_dict.cuh -- a dictionary trained from a batch of samples on the device (lz4f_mi355x_dev_trainDict).  The definition is the
// sequential statement in include/lz4f_mi355x.h (tests/train_model.py is the same in numpy): the corpus C is the valid samples back
// to back; every d-byte substring ("dmer") is hashed to f bits and counted; a window of m dmers scores the sum of the counts of its
// DISTINCT hashes; the window starts are dealt to E epochs; every round each epoch picks its best window against the counts as the
// round found them, and the picks are committed in epoch order against the live counts - a pick that has lost more than half its
// score to the picks in front of it is stale and waits for the next round.  The kernels:
//   k_td_scan     one workgroup (wg_scan_tile): the samples' lengths -> each sample's place in C (td_at, n_samples + 1 of them; a
//                 sample that gives nothing has no bytes there), the first invalid span, and the call's shape in TdCtl
//   k_td_gather   C, dealt by its own bytes: a thread takes 16 of them, bisects td_at for the first one's sample and walks on from there
//   k_td_hash     a thread per dmer: its hash (kept, 4 bytes per corpus byte) and the count (integer atomics: the totals are exact)
//   k_td_back     the look-back, once per call: min(j - prev(j), m) in 16 bits, prev(j) the last dmer in front of j with j's hash.
//                 A workgroup takes TD_TILE dmers with the m - 1 hashes in front of them in LDS
//   k_td_pick     a round's scores and picks.  Dmer j counts for exactly the starts [j - back(j) + 1, j]: a workgroup takes TD_TILE
//                 starts, adds every dmer that reaches them into a difference array in LDS (+count at its first start, -count behind
//                 its last) and scans it - O(1) per dmer instead of m gathers per start.  The best of an epoch: atomicMax over
//                 score << 32 | ~p, which prefers the lower start among equals (a score is at most M < 2^31: the sum of counts over
//                 DISTINCT hashes cannot exceed all the dmers there are)
//   k_td_commit   one workgroup, the picks in epoch order, its lanes over a pick's dmers: the live score, the trim, the copy to the
//                 dictionary's free end, the counts zeroed.  The last round's - the dictionary full, nothing appended, or `rounds`
//                 reached - zero-fills the front, writes the record and sets TdCtl::done: the kernels of later rounds return at once
// No kernel waits on another workgroup; the launch ladder is set-up and `rounds` times (pick, commit) whatever the samples hold.
#pragma once
#include "common.cuh"
#include "batch_common.cuh"

namespace lz4f {

constexpr uint32_t TD_TILE = LZ4F_MI355X_TRAIN_TILE, TD_THREADS = 256, TD_PER = TD_TILE / TD_THREADS;      // starts (dmers, bytes / 16) per thread and tile
constexpr uint32_t TD_MAX_K = 4096;
static_assert(TD_PER == 16 && TD_MAX_K <= TD_TILE, "k_td_gather takes 16 bytes a thread; k_td_back's halo is at most a tile");
constexpr uint64_t TD_PRIME = 0x9E3779B185EBCA87ull;
typedef uint64_t u64_ua __attribute__((aligned(1)));

struct TdCtl {                                           // the call's control block (device workspace, written by k_td_scan first)
    uint32_t done;                                       // the record is written: every later kernel returns at once
    uint32_t N, M, m, W, E;                              // the corpus' bytes; dmers, dmers to a window, window starts, epochs (N >= d)
    uint32_t first_bad;                                  // the first invalid span, BF_NONE: none
    uint32_t tail, n_seg, rounds_run;                    // the dictionary's free bytes, the segments appended, the rounds run
};
struct TdArgs { uint32_t k, d, f, rounds; };

__device__ __forceinline__ uint32_t td_hash(const uint8_t* __restrict__ c, uint32_t d, uint32_t f)
{
    uint64_t v = *(const u64_ua*)c;                                          // (C has 8 bytes of room behind its end)
    if (d < 8) v &= (1ull << (8 * d)) - 1;
    return (uint32_t)((v * TD_PRIME) >> (64 - f));
}

// by the whole workgroup, once: the front zero-filled, the record written, the call marked done
__device__ __forceinline__ void td_finish(TdCtl* __restrict__ ctl, uint8_t* __restrict__ dict, uint32_t dict_size, uint32_t tail, uint32_t n_seg,
                                          uint32_t rounds_run, ResultRec* __restrict__ rec)
{
    for (uint32_t i = threadIdx.x; i < tail; i += blockDim.x) dict[i] = 0;
    if (threadIdx.x == 0) {
        if (rec) {
            ResultRec x;
            x.size = dict_size - tail; x.consumed = ctl->N; x.status = ST_OK; x.n_blocks = n_seg; x.first_bad_block = ctl->first_bad;
            x.flags = (LZ4F_MI355X_PATH_BATCH << 12) | rounds_run;
            *rec = x;
        }
        ctl->tail = tail; ctl->n_seg = n_seg; ctl->rounds_run = rounds_run; ctl->done = 1;
    }
}

// sample i's valid length (0: an invalid span) - the one place the offsets are judged
__device__ __forceinline__ uint64_t td_span(const uint64_t* __restrict__ off, uint64_t src_bytes, uint32_t i, bool& bad)
{
    const uint64_t a = off[i], b = off[i + 1];
    bad = a > b || b > src_bytes;
    return bad ? 0 : b - a;
}

__global__ __launch_bounds__(1024) void k_td_scan(const uint64_t* __restrict__ off, uint64_t src_bytes, uint32_t n_samples, TdArgs a,
                                                  uint8_t* __restrict__ dict, uint32_t dict_size, uint64_t* __restrict__ at, TdCtl* __restrict__ ctl,
                                                  ResultRec* __restrict__ rec)
{
    __shared__ WgScan<1> s;
    __shared__ uint32_t sh_bad;
    __shared__ unsigned long long sh_n;
    if (threadIdx.x == 0) { sh_bad = BF_NONE; sh_n = 0; }
    wg_scan_begin(s);
    for (uint64_t base = 0; base < n_samples; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        bool bad = false;
        const uint64_t c[1] = {i < n_samples ? td_span(off, src_bytes, (uint32_t)i, bad) : 0u};
        uint64_t p[1];
        wg_scan_tile(c, p, s);
        if (i < n_samples) {
            // (the sums only grow: once a sample does not fit, none behind it does, an empty one at a place beyond srcBytes included)
            const bool fits = p[0] + c[0] <= src_bytes;
            if (fits) atomicMax(&sh_n, (unsigned long long)(p[0] + c[0]));
            at[i] = fits ? p[0] : ~0ull;
            if (bad) atomicMin(&sh_bad, (uint32_t)i);
        }
    }
    __syncthreads();
    const uint64_t N = sh_n;
    // a sample that was dropped lies at N with no bytes, as does the end: td_at is monotone, and k_td_gather bisects it
    for (uint64_t i = threadIdx.x; i <= n_samples; i += 1024) if (i == n_samples || at[i] == ~0ull) at[i] = N;
    __syncthreads();
    if (threadIdx.x == 0) {
        TdCtl c;
        c.done = 0; c.N = (uint32_t)N; c.first_bad = sh_bad; c.tail = dict_size; c.n_seg = 0; c.rounds_run = 0;
        c.M = N >= a.d ? (uint32_t)N - a.d + 1 : 0;
        c.m = min(a.k - a.d + 1, c.M);
        c.W = c.M - c.m + 1;
        c.E = max(1u, min(dict_size / a.k, c.W));
        *ctl = c;
    }
    __syncthreads();
    if (N < a.d) td_finish(ctl, dict, dict_size, dict_size, 0, 0, rec);                        // no dmer: all zeros
}

__global__ __launch_bounds__(TD_THREADS) void k_td_gather(const uint8_t* __restrict__ src, const uint64_t* __restrict__ off, uint32_t n_samples,
                                                          const uint64_t* __restrict__ at, const TdCtl* __restrict__ ctl, uint8_t* __restrict__ C)
{
    if (ctl->done) return;
    const uint64_t N = ctl->N;
    for (uint64_t q0 = ((uint64_t)blockIdx.x * TD_THREADS + threadIdx.x) * 16; q0 < N; q0 += (uint64_t)gridDim.x * TD_TILE) {
        uint32_t lo = 0, hi = n_samples;                                     // at[lo] <= q0 < at[hi]  (at[0] = 0, at[n_samples] = N)
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (at[mid] <= q0) lo = mid; else hi = mid; }
        uint32_t i = lo;
        uint64_t end = at[i + 1], from = off[i] - at[i];                     // sample i's bytes: src[from + q] for q in [at[i], end)
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t b = 0; b < 16 && q0 + b < N; b++) {
            const uint64_t q = q0 + b;
            while (q >= end) { i++; end = at[i + 1]; from = off[i] - at[i]; }                  // (q < N = at[n_samples]: it ends)
            w[b >> 2] |= (uint32_t)src[from + q] << (8 * (b & 3));
        }
        *(uint4*)(C + q0) = make_uint4(w[0], w[1], w[2], w[3]);              // (C is 16-byte aligned with 16 bytes of room behind N)
    }
}

__global__ __launch_bounds__(TD_THREADS) void k_td_hash(const uint8_t* __restrict__ C, const TdCtl* __restrict__ ctl, TdArgs a, uint32_t* __restrict__ hv,
                                                        uint32_t* __restrict__ freq)
{
    if (ctl->done) return;
    const uint32_t M = ctl->M;
    for (uint64_t j = (uint64_t)blockIdx.x * TD_THREADS + threadIdx.x; j < M; j += (uint64_t)gridDim.x * TD_THREADS) {
        const uint32_t h = td_hash(C + j, a.d, a.f);
        hv[j] = h;
        atomicAdd(&freq[h], 1u);
    }
}

__global__ __launch_bounds__(TD_THREADS) void k_td_back(const uint32_t* __restrict__ hv, const TdCtl* __restrict__ ctl, uint16_t* __restrict__ back)
{
    __shared__ uint32_t s_h[2 * TD_TILE];                                    // the tile's hashes at [TD_TILE, 2 TD_TILE), the halo in front
    if (ctl->done) return;
    const uint32_t M = ctl->M, m = ctl->m, halo = m - 1;                     // (m <= TD_MAX_K - 3: the halo fits)
    for (uint64_t t0 = (uint64_t)blockIdx.x * TD_TILE; t0 < M; t0 += (uint64_t)gridDim.x * TD_TILE) {
        const uint32_t n = (uint32_t)min((uint64_t)TD_TILE, M - t0), reach = (uint32_t)min((uint64_t)halo, t0);
        for (uint32_t i = threadIdx.x; i < reach + n; i += TD_THREADS) s_h[TD_TILE - reach + i] = hv[t0 - reach + i];
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += TD_THREADS) {
            const uint32_t h = s_h[TD_TILE + i], most = min(halo, reach + i);                  // dmers in front of j that a window can share with it
            uint32_t t = 1;
            while (t <= most && s_h[TD_TILE + i - t] != h) t++;
            // (none within m - 1: prev(j) is further than a window reaches, or there is none - then j - prev(j) = j + 1)
            back[t0 + i] = (uint16_t)(t <= most ? t : (uint32_t)min((uint64_t)m, t0 + i + 1));
        }
        __syncthreads();
    }
}

// the epoch of start p: the largest e with e * W / E <= p
__device__ __forceinline__ uint32_t td_epoch(uint32_t p, uint32_t W, uint32_t E) { return (uint32_t)((((uint64_t)p + 1) * E - 1) / W); }
__device__ __forceinline__ uint32_t td_epoch_begin(uint32_t e, uint32_t W, uint32_t E) { return (uint32_t)((uint64_t)e * W / E); }

__global__ __launch_bounds__(TD_THREADS) void k_td_pick(const uint32_t* __restrict__ hv, const uint16_t* __restrict__ back, const uint32_t* __restrict__ freq,
                                                        const TdCtl* __restrict__ ctl, unsigned long long* __restrict__ best)
{
    __shared__ unsigned long long s_diff[TD_TILE + 1];
    __shared__ uint64_t s_w[TD_THREADS / WAVE];
    if (ctl->done) return;
    const uint32_t M = ctl->M, m = ctl->m, W = ctl->W, E = ctl->E;
    for (uint64_t t0 = (uint64_t)blockIdx.x * TD_TILE; t0 < W; t0 += (uint64_t)gridDim.x * TD_TILE) {
        for (uint32_t i = threadIdx.x; i <= TD_TILE; i += TD_THREADS) s_diff[i] = 0;
        __syncthreads();
        const uint64_t t1 = t0 + TD_TILE, j_end = min((uint64_t)M, t1 + m - 1);                // the dmers that reach a start of [t0, t1)
        for (uint64_t j = t0 + threadIdx.x; j < j_end; j += TD_THREADS) {
            const uint32_t v = freq[hv[j]];
            if (!v) continue;
            const uint64_t first = j + 1 - back[j], lo = max(first, t0), hi = min(j, t1 - 1);
            if (lo > hi) continue;
            atomicAdd(&s_diff[lo - t0], (unsigned long long)v);
            atomicAdd(&s_diff[hi + 1 - t0], 0ull - v);
        }
        __syncthreads();
        // the scan: a thread's 16 starts, the wave's threads, the waves
        uint64_t sc[TD_PER], sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < TD_PER; q++) { sum += s_diff[threadIdx.x * TD_PER + q]; sc[q] = sum; }
        uint64_t incl = sum;
        for (uint32_t dd = 1; dd < WAVE; dd <<= 1) { const uint64_t x = __shfl_up(incl, dd); if (lane_id() >= dd) incl += x; }
        if (lane_id() == WAVE - 1) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint64_t before = incl - sum;
        for (uint32_t q = 0; q < (threadIdx.x >> 6); q++) before += s_w[q];
        // the thread's starts are consecutive: one atomic per epoch they touch
        const uint64_t p0 = t0 + threadIdx.x * TD_PER;
        if (p0 < W) {
            uint32_t e = td_epoch((uint32_t)p0, W, E);
            uint64_t next = e + 1 < E ? td_epoch_begin(e + 1, W, E) : W;
            unsigned long long key = 0;
#pragma unroll
            for (uint32_t q = 0; q < TD_PER; q++) {
                const uint64_t p = p0 + q;
                if (p < W) {
                    while (p >= next) { atomicMax(&best[e], key); key = 0; e++; next = e + 1 < E ? td_epoch_begin(e + 1, W, E) : W; }
                    const unsigned long long mine = ((before + sc[q]) << 32) | (0xFFFFFFFFu - (uint32_t)p);
                    key = max(key, mine);
                }
            }
            atomicMax(&best[e], key);
        }
        __syncthreads();
    }
}

// the workgroup's sum, minimum and maximum at once (every thread gets them; `slot` alternates so that one barrier a call suffices)
struct TdRed { uint64_t sum; uint32_t lo, hi; };
__device__ __forceinline__ TdRed td_reduce(TdRed v, TdRed (&s)[2][TD_THREADS / WAVE], uint32_t slot)
{
#pragma unroll
    for (int sft = 1; sft < WAVE; sft <<= 1) {
        v.sum += __shfl_xor(v.sum, sft);
        v.lo = min(v.lo, (uint32_t)__shfl_xor(v.lo, sft));
        v.hi = max(v.hi, (uint32_t)__shfl_xor(v.hi, sft));
    }
    if (lane_id() == 0) s[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    TdRed r = s[slot][0];
#pragma unroll
    for (uint32_t q = 1; q < TD_THREADS / WAVE; q++) { const TdRed x = s[slot][q]; r.sum += x.sum; r.lo = min(r.lo, x.lo); r.hi = max(r.hi, x.hi); }
    return r;
}

__global__ __launch_bounds__(TD_THREADS) void k_td_commit(const uint8_t* __restrict__ C, const uint32_t* __restrict__ hv, const uint16_t* __restrict__ back,
                                                          uint32_t* __restrict__ freq, TdCtl* __restrict__ ctl, unsigned long long* __restrict__ best, TdArgs a,
                                                          uint32_t last, uint8_t* __restrict__ dict, uint32_t dict_size, ResultRec* __restrict__ rec)
{
    __shared__ TdRed s_red[2][TD_THREADS / WAVE];
    if (ctl->done) return;
    const uint32_t m = ctl->m, E = ctl->E;
    uint32_t tail = ctl->tail, n_seg = ctl->n_seg, appended = 0, slot = 0;                   // (uniform: every thread keeps them)
    for (uint32_t e = 0; e < E && tail; e++) {
        const unsigned long long key = best[e];
        const uint64_t snap = key >> 32;
        if (!snap) continue;
        const uint32_t p = 0xFFFFFFFFu - (uint32_t)key;
        TdRed v; v.sum = 0; v.lo = 0xFFFFFFFFu; v.hi = 0;
        for (uint32_t i = threadIdx.x; i < m; i += TD_THREADS) {
            const uint32_t j = p + i, fr = freq[hv[j]];
            if (fr) { v.lo = min(v.lo, j); v.hi = max(v.hi, j); if (back[j] > i) v.sum += fr; }                 // (back > i: prev(j) < p)
        }
        v = td_reduce(v, s_red, slot);
        slot ^= 1;
        if (2 * v.sum < snap) continue;                                                        // stale: the next round picks afresh
        const uint32_t s0 = v.lo, s1 = v.hi, take = min(s1 + a.d - s0, tail);                  // (snap > 0 and not stale: some dmer counts)
        for (uint32_t i = threadIdx.x; i < take; i += TD_THREADS) dict[tail - take + i] = C[s0 + i];
        for (uint32_t j = s0 + threadIdx.x; j <= s1; j += TD_THREADS) freq[hv[j]] = 0;
        tail -= take; n_seg++; appended++;
        __syncthreads();                                                                       // the next pick reads the counts as this one left them
    }
    const uint32_t rounds_run = ctl->rounds_run + 1;
    __syncthreads();
    if (!tail || !appended || last) { td_finish(ctl, dict, dict_size, tail, n_seg, rounds_run, rec); return; }
    for (uint32_t e = threadIdx.x; e < E; e += TD_THREADS) best[e] = 0;
    if (threadIdx.x == 0) { ctl->tail = tail; ctl->n_seg = n_seg; ctl->rounds_run = rounds_run; }
}

}  // namespace lz4f
