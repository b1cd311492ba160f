// batch_common.cuh -- what the "many frames in one device call" paths share (decode_batch.cuh, measure_batch.cuh, encode_batch.cuh):
//   wg_scan_tile       the 1024-thread tiled exclusive scan with a carry, over N quantities at once
//   k_batch_place      one workgroup: the scan of the frames' block counts -> each frame's slice of the block table (decode, measure)
//   BatchCore          the decode-side frame record; batch_frame_head fills it: a frame's grammar from "the span is valid" to "the
//                      record is complete" (frame_format.hpp: skippable frames, header, size words, EndMark, content checksum word),
//                      the caller's bound on the blocks and its per-block predicate as callables
//   bf_walk            the walk over a frame's size words; batch_table_walk: a placed frame's words walked again, for its entries
//   slice_holds        "an entry of this call: its frame's slice holds it"
//   slice_verdict      a wave over a frame's table slice: the first block that failed, and the sum of the others
#pragma once
#include "common.cuh"
#include "frame_dev.cuh"

namespace lz4f {

constexpr uint32_t BF_NONE = 0xFFFFFFFFu;   // no table slice; no block

// ---- the scan ----
template <int N>
struct WgScan {                             // the scan's LDS (the caller's __shared__)
    uint64_t wsum[N][16];
    uint64_t carry[N];                      // the totals of the tiles so far: every thread may read them between two tiles and after the last
};
template <int N>
__device__ __forceinline__ void wg_scan_begin(WgScan<N>& s)
{
    if (threadIdx.x < N) s.carry[threadIdx.x] = 0;
    __syncthreads();
}
// One tile of 1024 threads: c[k] is this thread's count of quantity k (0 beyond the end) -> at[k], its exclusive prefix over this
// tile and all the tiles before.  Three barriers a tile whatever N is; the whole workgroup calls it.
template <int N>
__device__ __forceinline__ void wg_scan_tile(const uint64_t (&c)[N], uint64_t (&at)[N], WgScan<N>& s)
{
    const uint32_t t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    uint64_t incl[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        incl[k] = c[k];
        for (uint32_t d = 1; d < WAVE; d <<= 1) { const uint64_t x = __shfl_up(incl[k], d); if (lane >= d) incl[k] += x; }
        if (lane == WAVE - 1) s.wsum[k][wv] = incl[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        uint64_t before = s.carry[k];
        for (uint32_t q = 0; q < wv; q++) before += s.wsum[k][q];
        at[k] = before + incl[k] - c[k];
    }
    __syncthreads();
    if (t == 1023) {
#pragma unroll
        for (int k = 0; k < N; k++) s.carry[k] = at[k] + c[k];
    }
    __syncthreads();
}

// ---- the table slices ----
// an entry w of this call: the slice [at, at + n) of its frame holds it.  What an earlier, larger batch left in a table is not: no
// frame's slice holds it, or the frame it names has its slice elsewhere.  (The caller has checked the entry's frame number against
// n_frames, and asks for the frame's status where a failed frame can own a slice.)
__device__ __forceinline__ bool slice_holds(uint32_t at, uint32_t n, uint32_t w)
{
    return at != BF_NONE && w >= at && w - at < n;
}

// one workgroup: exclusive scan of the counts -> frames[i].tbl_at.  A frame whose slice would end beyond the table keeps BF_NONE (the
// caller's serial kernel takes it) and still counts.  ctl[0]: the entries in use
template <typename FrameT>
__global__ __launch_bounds__(1024) void k_batch_place(const uint32_t* __restrict__ counts, uint32_t n_frames, FrameT* __restrict__ frames,
                                                      uint64_t table_cap, uint32_t* __restrict__ ctl)
{
    __shared__ WgScan<1> s;
    wg_scan_begin(s);
    for (uint32_t base = 0; base < n_frames; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t c[1] = {i < n_frames ? counts[i] : 0u};
        uint64_t at[1];
        wg_scan_tile(c, at, s);
        if (c[0] && at[0] + c[0] <= table_cap) frames[i].tbl_at = (uint32_t)at[0];
    }
    if (threadIdx.x == 0) ctl[0] = (uint32_t)(s.carry[0] < table_cap ? s.carry[0] : table_cap);
}

// by one wave, over the n entries of a slice: bad, the first block b with got(b) < 0 (BF_NONE: none), kind, its got, and sum, the
// sum of the got(b) > 0.  got(b) is called by all 64 lanes together, lane l with b = 64 * k + l, and returns 0 where b >= n.
template <typename G>
__device__ __forceinline__ void slice_verdict(uint32_t n, uint32_t& bad, int32_t& kind, uint64_t& sum, G&& got)
{
    bad = BF_NONE; kind = 0; sum = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += WAVE) {
        const int32_t g = got(b0 + lane_id());
        const uint64_t fm = __ballot(g < 0);
        if (fm && bad == BF_NONE) { bad = b0 + (uint32_t)__builtin_ctzll(fm); kind = (int32_t)__shfl((uint32_t)g, (int)(bad - b0)); }
        uint64_t s = g > 0 ? (uint64_t)g : 0u;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) s += __shfl_xor(s, sft);
        sum += s;
    }
}

// ---- the frames ----
struct BatchCore {                          // per frame (device workspace, 64 bytes)
    uint64_t src, span;                     // the frame's span in d_src
    uint64_t consumed, size;                // as the result record (size: the declared content size until the verdict)
    uint32_t status, flags, n_blocks, first_bad;
    uint32_t bs, hsize, tbl_at, last;       // tbl_at: first table entry, BF_NONE: the serial kernel takes the frame; last: measure_batch.cuh
};

// The walk over a frame's size words, from `pos` (the first word) to behind the EndMark: each(w, csz, at) for block b with size
// word w and csz payload bytes at f + at; what it returns, if not ST_OK, ends the walk and is the walk's status, as the grammar's
// own errors are.  b: the blocks walked (on an error: the block it ended at).  UNI: a wave walks (the words are wave-uniform).
template <bool UNI, typename F>
__device__ __forceinline__ uint32_t bf_walk(const uint8_t* __restrict__ f, uint64_t cap, uint64_t& pos, uint32_t& b, uint32_t bs, uint32_t bck, F&& each)
{
    for (b = 0;; b++) {
        if (!frame_word_fits(cap - pos)) return ST_INCOMPLETE;
        const uint32_t w = UNI ? uni(rd32le(f + pos)) : rd32le(f + pos);
        pos += 4;
        if (is_endmark(w)) return ST_OK;
        uint32_t csz; uint64_t step;
        if (const uint32_t st = frame_block_word(w, bs, bck, cap - pos, csz, step)) return st;
        const uint64_t at = pos;
        pos += step;                                              // (first: nothing of this hop is alive while `each` works)
        if (const uint32_t st = each(w, csz, at)) return st;
    }
}

// BatchCore's initial state: nothing read, no slice
__device__ __forceinline__ void batch_core_init(BatchCore& r, uint64_t src)
{
    r.src = src; r.span = 0; r.consumed = 0; r.size = 0;
    r.status = 0; r.flags = 0; r.n_blocks = 0; r.first_bad = BF_NONE; r.bs = 0; r.hsize = 0; r.tbl_at = BF_NONE; r.last = 0;
}

// One thread, one frame, r.src and r.span valid: the single call's walk (k_walk_frame), check for check -> the frame's status, and r
// filled as far as the walk came (all of it but status and tbl_at when ST_OK).  bound(bs): the most blocks the caller takes, more is
// ERROR_dstMaxSize_tooSmall; each(bs): the caller's say on one more block, ST_OK or the frame's status.
template <typename Bound, typename Each>
__device__ __forceinline__ uint32_t batch_frame_head(const uint8_t* __restrict__ src, BatchCore& r, Bound&& bound, Each&& each)
{
    const uint8_t* f = src + r.src;
    const uint64_t cap = r.span;
    if (cap < 7) return ST_INCOMPLETE;
    if (is_skippable(rd32le(f))) {                                                      // no output
        if (const uint32_t st = skippable_span(f, cap, r.consumed)) { r.consumed = 0; return st; }
        r.flags = FLAG_SKIPPABLE;
        return ST_OK;
    }
    FrameHead h;
    if (const uint32_t st = frame_head_parse(f, cap, h)) return st;
    r.flags = h.flg; r.bs = h.bs; r.hsize = h.hsize;
    uint64_t tcap = bound(h.bs);
    if (tcap > 0x7FFFFFFFull) tcap = 0x7FFFFFFFull;
    uint64_t pos = h.hsize;
    uint32_t n = 0;
    if (const uint32_t st = bf_walk<false>(f, cap, pos, n, h.bs, h.bck, [&](uint32_t, uint32_t, uint64_t) -> uint32_t {
            return n >= tcap ? (uint32_t)ST_DSTSMALL : each(h.bs);
        })) return st;
    uint32_t tail;
    if (const uint32_t st = frame_end(h.flg, cap - pos, tail)) return st;
    r.n_blocks = n; r.consumed = pos + tail; r.size = h.content;
    return ST_OK;
}

// A thread per frame (workgroups of 256): a frame that has a slice walks its size words again, entry(i, r, b, w, at) for block b of
// frame i with size word w and its payload at r.src + at - the caller's table entry
template <typename FrameT, typename F>
__device__ __forceinline__ void batch_table_walk(const uint8_t* __restrict__ src, const FrameT* __restrict__ frames, uint32_t n_frames, F&& entry)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    const FrameT r = frames[i];
    if (r.status != 0 || r.tbl_at == BF_NONE) return;
    uint64_t pos = r.hsize;
    uint32_t b;
    bf_walk<false>(src + r.src, r.span, pos, b, r.bs, flg_bck(r.flags), [&](uint32_t w, uint32_t, uint64_t at) -> uint32_t {
        if (b >= r.n_blocks) return ST_GENERIC;                 // (the head kernel walked this frame: it has n_blocks of them)
        entry(i, r, b, w, at);
        return ST_OK;
    });
}

}  // namespace lz4f
