// pack_batch.cuh -- a batch's frames back to back in one stream (lz4f_mi355x_dev_packFrames), and the stream's own frame directory
// read back into offsets (lz4f_mi355x_dev_readPackDirectory).  No frame byte is parsed: the lengths are what the compress call's
// records say, held to the windows they came from.
//   k_pk_scan     one workgroup (wg_scan_tile): L[i] from record i and its window -> d_dst_off, the verdict (ctl[0]), the pack record;
//                 and, once the verdict is 0, the directory: its fixed part and the L array (frame_format.hpp: pack_dir_*)
//   k_pk_copy     the copy, dealt by OUTPUT bytes: a workgroup takes tiles of LZ4F_MI355X_PACK_TILE output bytes, striding; the tile's
//                 frames by search in d_dst_off (the tile's first and last frame by a wave, 64 probes a step; a unit's frame between
//                 them by bisection); a lane's unit is 16 bytes aligned to the DESTINATION address.  A unit inside one
//                 frame: one unaligned 16-byte load, one aligned 16-byte store, PK_UNITS of them in flight per lane.  A unit that
//                 straddles frames (several of them may be empty, or 11 bytes long), the stream's head behind the directory and its tail:
//                 byte by byte.  Every load lies inside the frame it copies; nothing happens unless the verdict is 0
//   k_pk_readdir  one workgroup: the directory's fixed part and its sums, every read bounded by packBytes -> the offsets, or n + 1 zeros
#pragma once
#include "common.cuh"
#include "batch_common.cuh"

namespace lz4f {

constexpr uint32_t PK_TILE = LZ4F_MI355X_PACK_TILE, PK_THREADS = 256, PK_UNITS = PK_TILE / 16 / PK_THREADS;      // units per lane and tile
static_assert(PK_UNITS * PK_THREADS * 16 == PK_TILE && PK_UNITS >= 1, "pack tile");
constexpr uint32_t PK_PER = 2;              // frames per thread and tile of the two scans: 2048 frames between two carries

// frame i's length: its record's size when the record says status 0 and offsets and size hold; 0 otherwise.  lies: status 0, but they do not
__device__ __forceinline__ uint64_t pk_len(const ResultRec* __restrict__ results, const uint64_t* __restrict__ soff, uint64_t src_bytes, uint32_t i, bool& lies)
{
    const uint32_t status = results[i].status;                                                // (all four loads at once: none waits for another)
    const uint64_t s0 = soff[i], s1 = soff[i + 1], size = results[i].size;
    lies = status == 0 && !(s0 <= s1 && s1 <= src_bytes && size <= s1 - s0);
    return status != 0 || lies ? 0 : size;
}

// a u32 of the directory: it may stand at any alignment
__device__ __forceinline__ void pk_put32(uint8_t* p, uint32_t v)
{
    if (((uintptr_t)p & 3u) == 0) *(uint32_t*)p = v; else st32le(p, v);
}

// dir: the directory is asked for.  doff is written, then read by other threads behind a barrier (one workgroup: one L1)
__global__ __launch_bounds__(1024) void k_pk_scan(const ResultRec* __restrict__ results, const uint64_t* __restrict__ soff, uint64_t src_bytes, uint32_t n_frames,
                                                  uint8_t* __restrict__ dst, uint64_t dst_bytes, uint64_t* doff, uint32_t dir,
                                                  uint32_t* __restrict__ ctl, ResultRec* __restrict__ rec)
{
    __shared__ WgScan<2> s;
    __shared__ uint32_t sh_bad, sh_big;
    if (threadIdx.x == 0) { sh_bad = BF_NONE; sh_big = 0; }
    wg_scan_begin(s);
    const uint64_t D = dir ? pack_dir_size(n_frames) : 0;
    // a thread takes PK_PER consecutive frames of a tile (fewer tiles, and so fewer barriers, for the same frames); the next tile's
    // loads fly while this one is scanned
    uint64_t L[PK_PER], L_next[PK_PER];
    uint32_t lies = 0, lies_next = 0;                                                         // bit j: frame i0 + j
    auto fetch = [&](uint64_t i0, uint64_t (&len)[PK_PER], uint32_t& mask) {
        mask = 0;
#pragma unroll
        for (uint32_t j = 0; j < PK_PER; j++) {
            bool x = false;
            len[j] = i0 + j < n_frames ? pk_len(results, soff, src_bytes, (uint32_t)(i0 + j), x) : 0;
            mask |= (uint32_t)x << j;
        }
    };
    fetch((uint64_t)threadIdx.x * PK_PER, L, lies);
    for (uint64_t base = 0; base < n_frames; base += 1024 * PK_PER) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * PK_PER;
        fetch(i0 + 1024 * PK_PER, L_next, lies_next);
        uint64_t c[2] = {0, 0}, at[2];
#pragma unroll
        for (uint32_t j = 0; j < PK_PER; j++) {
            if ((lies >> j) & 1u) atomicMin(&sh_bad, (uint32_t)(i0 + j));
            if (L[j] > 0xFFFFFFFFull) sh_big = 1;
            c[0] += L[j]; c[1] += L[j] ? 1u : 0u;
        }
        wg_scan_tile(c, at, s);
        uint64_t run = D + at[0];
#pragma unroll
        for (uint32_t j = 0; j < PK_PER; j++) {
            if (i0 + j < n_frames) doff[i0 + j] = run;
            run += L[j];
            L[j] = L_next[j];
        }
        lies = lies_next;
    }
    const uint64_t sum = s.carry[0], total = D + sum;
    uint32_t verdict = ST_OK;
    if (dir && (sh_big || n_frames > PACKDIR_MOST)) verdict = ST_SRCLARGE;              // a length, or the payload's size, that a u32 cannot say
    if (total > dst_bytes) verdict = ST_DSTSMALL;
    if (threadIdx.x == 0) {
        doff[n_frames] = total;
        ctl[0] = verdict;
        if (rec) {
            ResultRec x;
            x.size = total; x.consumed = sum; x.status = verdict; x.n_blocks = (uint32_t)s.carry[1]; x.first_bad_block = sh_bad;
            x.flags = LZ4F_MI355X_PATH_BATCH;
            *rec = x;
        }
    }
    if (!dir || verdict != ST_OK) return;
    if (threadIdx.x == 0) pack_dir_head_write(dst, n_frames, sum);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_frames; i += 1024) pk_put32(dst + pack_dir_len_at(i), (uint32_t)(doff[i + 1] - doff[i]));
}

// the greatest i in [a, b] with off[i] <= p (off[a] <= p is the caller's), by a whole wave for wave-uniform a, b and p: the lanes probe
// 64 places of (a, b] at once, so a step divides the range by 64 where a binary search halves it - two dependent loads for 4096 frames
__device__ __forceinline__ uint32_t pk_frame_of(const uint64_t* __restrict__ off, uint32_t a, uint32_t b, uint64_t p)
{
    while (a < b) {
        const uint32_t step = (b - a + WAVE - 1) / WAVE;                                       // lane l probes a + (l + 1) * step, b at most
        const uint64_t m = (uint64_t)a + (uint64_t)(lane_id() + 1) * step;
        const uint32_t hits = (uint32_t)__builtin_popcountll(__ballot(off[m < b ? m : b] <= p));   // (off ascends: the first `hits` lanes)
        if (hits == WAVE) return b;                                                            // (the last lane probes b)
        const uint64_t last = (uint64_t)a + (uint64_t)hits * step, miss = last + step;         // the last hit (a itself: none), the first miss
        b = uni((uint32_t)(miss < b ? miss : b) - 1);
        a = uni((uint32_t)last);
    }
    return a;
}

// Unit u is the output bytes [16 * u - shift, 16 * u - shift + 16) with shift = dst & 15, cut to [D, total): D = doff[0] (the directory
// is k_pk_scan's), total = doff[n_frames].  Tile t is the units [t * PK_TILE / 16, (t + 1) * PK_TILE / 16).  The grid is sized from
// the host's bound on the output and capped: the workgroups stride over the tiles in use.  n_frames >= 1.
__global__ __launch_bounds__(PK_THREADS) void k_pk_copy(const uint8_t* __restrict__ src, const uint64_t* __restrict__ soff, uint32_t n_frames,
                                                        uint8_t* __restrict__ dst, const uint64_t* __restrict__ doff, const uint32_t* __restrict__ ctl)
{
    if (ctl[0] != ST_OK) return;
    const uint64_t D = doff[0], total = doff[n_frames];
    if (total <= D) return;
    const uint64_t shift = (uintptr_t)dst & 15u;
    constexpr uint64_t TU = PK_TILE / 16;
    const uint64_t tile_from = (D + shift) / 16 / TU, tile_to = ((total + shift + 15) / 16 + TU - 1) / TU;
    for (uint64_t tile = tile_from + blockIdx.x; tile < tile_to; tile += gridDim.x) {
        // the tile's output bytes [p_lo, p_hi) and the frames they fall in (the same for every lane)
        const uint64_t t0 = tile * PK_TILE, t1 = t0 + PK_TILE;                              // (in shifted positions: p + shift)
        const uint64_t p_lo = t0 > D + shift ? t0 - shift : D, p_hi = t1 - shift < total ? t1 - shift : total;
        const uint32_t f_lo = pk_frame_of(doff, 0, n_frames - 1, p_lo), f_hi = pk_frame_of(doff, f_lo, n_frames - 1, p_hi - 1);
        uint64_t lo[PK_UNITS], hi[PK_UNITS];
        uint32_t fr[PK_UNITS];
        bool whole[PK_UNITS];
        b16_ua v[PK_UNITS];
        // ---- the units' frames: pk_frame_of for all of a lane's units at once, a step (the tile's frames halved) for each together ----
        uint32_t top[PK_UNITS];
#pragma unroll
        for (uint32_t k = 0; k < PK_UNITS; k++) {
            const uint64_t q = t0 + 16ull * (k * PK_THREADS + threadIdx.x);                    // the unit's first byte, shifted
            lo[k] = q > D + shift ? q - shift : D;
            hi[k] = q + 16 - shift < total ? q + 16 - shift : total;
            if (lo[k] >= hi[k]) lo[k] = hi[k] = p_lo;                                         // (in front of the head, or behind the tail: nothing)
            fr[k] = f_lo; top[k] = f_hi;
        }
        for (uint32_t span = f_hi - f_lo; span; span >>= 1) {
#pragma unroll
            for (uint32_t k = 0; k < PK_UNITS; k++) {
                const uint32_t m = fr[k] + (top[k] - fr[k] + 1) / 2;                          // (== fr[k] once the two have met)
                if (doff[m] <= lo[k]) fr[k] = m; else top[k] = m - 1;
            }
        }
        // ---- the loads of the units that lie inside one frame, all of them before the first store ----
        uint64_t from[PK_UNITS];
#pragma unroll
        for (uint32_t k = 0; k < PK_UNITS; k++) {
            whole[k] = hi[k] - lo[k] == 16 && doff[fr[k] + 1] >= hi[k];
            from[k] = soff[fr[k]] + (lo[k] - doff[fr[k]]);
        }
#pragma unroll
        for (uint32_t k = 0; k < PK_UNITS; k++) {
            v[k] = b16_ua{0, 0, 0, 0};
            if (whole[k]) v[k] = *(const b16_ua*)(src + from[k]);
        }
#pragma unroll
        for (uint32_t k = 0; k < PK_UNITS; k++)
            if (whole[k]) *(uint4*)(dst + lo[k]) = uint4{v[k].a, v[k].b, v[k].c, v[k].d};   // (dst + lo is 16-byte aligned: lo + shift = q)
        // ---- the others, byte by byte: a frame's end, the frames behind it (empty ones too), the stream's head and tail ----
#pragma unroll
        for (uint32_t k = 0; k < PK_UNITS; k++) {
            if (whole[k]) continue;
            uint32_t f = fr[k];
            for (uint64_t p = lo[k]; p < hi[k];) {                                             // a frame's share of the unit at a time
                while (doff[f + 1] <= p) f++;                                                  // (p < total = doff[n_frames]: f stays below n_frames)
                const uint64_t e = doff[f + 1] < hi[k] ? doff[f + 1] : hi[k];
                const uint32_t nb = (uint32_t)(e - p);                                         // 1 .. 16
                const uint8_t* sp = src + soff[f] + (p - doff[f]);
                uint8_t b[16];
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) if (j < nb) b[j] = sp[j];
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) if (j < nb) dst[p + j] = b[j];
                p = e;
            }
        }
    }
}

// The directory in pack[0 .. pack_bytes) against the caller's n_frames -> off: D, then the running sums; or n_frames + 1 zeros and why.
__global__ __launch_bounds__(1024) void k_pk_readdir(const uint8_t* __restrict__ pack, uint64_t pack_bytes, uint32_t n_frames, uint64_t* __restrict__ off,
                                                     ResultRec* __restrict__ rec)
{
    __shared__ WgScan<1> s;
    wg_scan_begin(s);
    const uint64_t D = pack_dir_size(n_frames);
    uint32_t stored = 0;
    uint64_t frames_bytes = 0, sum = 0;
    uint32_t st = pack_dir_head_parse(pack, pack_bytes, stored, frames_bytes);
    if (!st && stored != n_frames) st = ST_FRAMESIZE;
    if (!st && pack_bytes < D) st = ST_INCOMPLETE;
    if (!st) {
        for (uint32_t base = 0; base < n_frames; base += 1024 * PK_PER) {                      // (n_frames <= PACKDIR_MOST here: no wrap)
            const uint32_t i0 = base + threadIdx.x * PK_PER;
            uint32_t len[PK_PER];
            uint64_t c[1] = {0}, at[1];
#pragma unroll
            for (uint32_t j = 0; j < PK_PER; j++) { len[j] = i0 + j < n_frames ? rd32le(pack + pack_dir_len_at(i0 + j)) : 0u; c[0] += len[j]; }
            wg_scan_tile(c, at, s);
            uint64_t run = D + at[0];
#pragma unroll
            for (uint32_t j = 0; j < PK_PER; j++) { if (i0 + j < n_frames) off[i0 + j] = run; run += len[j]; }
        }
        sum = s.carry[0];
        if (sum != frames_bytes) st = ST_FRAMESIZE;
        else if (frames_bytes > pack_bytes - D) st = ST_INCOMPLETE;                            // (the frames are not all here)
    }
    if (st) {
        __syncthreads();                                                                      // (other threads' offsets are written over)
        for (uint64_t i = threadIdx.x; i <= n_frames; i += 1024) off[i] = 0;
    } else if (threadIdx.x == 0) off[n_frames] = D + sum;
    if (threadIdx.x == 0 && rec) {
        ResultRec x;
        x.size = st ? 0 : frames_bytes; x.consumed = st ? 0 : D + frames_bytes; x.status = st; x.n_blocks = st ? 0 : n_frames;
        x.first_bad_block = BF_NONE; x.flags = LZ4F_MI355X_PATH_BATCH;
        *rec = x;
    }
}

}  // namespace lz4f
