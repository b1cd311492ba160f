// split_batch.cuh -- the frame boundaries of a concatenated LZ4 stream, found on the device (lz4f_mi355x_dev_splitFrames).  The
// definition is the serial walk (sp_step by sp_step from byte 0: k_split_serial runs it verbatim); the parallel kernels give the
// same answer without the chain of dependent reads from frame to frame:
//   k_sp_cand     every byte position is looked at once (a streaming read, 16-byte loads, four in flight per thread): a position is a
//                 NODE when its four bytes are FRAME_MAGIC and frame_head_parse accepts the header in the bytes that remain, or a
//                 skippable magic whose 8-byte head and payload fit.  Position 0 is always a node, the root.  A bit per position
//                 (a u16 per 16-byte unit) and a count per SP_CHUNK bytes
//   k_sp_order    one workgroup (wg_scan_tile): the chunks' counts -> each chunk's place in the node list; more nodes than the list
//                 holds (sp_node_cap, from the call's arguments alone): overflow, k_split_serial delivers
//   k_sp_list     the bits -> the node list, in position order
//   k_sp_extent   a thread per node: sp_step, the model's step, at the node (header, size words by bf_walk, EndMark, checksum word)
//                 -> where its frame ends, or why it does not; the end looked up in the list by bisection -> the node's link: another
//                 node, or none (the end is srcBytes, or no node, or there is no end)
//   k_sp_double   the true frames are the nodes REACHABLE from the root: pointer doubling over the links, sp_rounds(capacity) rounds
//                 of one launch each.  (Not "the list is a gap-free chain", as k_walk_link asks of block starts: a .lz4 file inside
//                 a stored block is a perfect false node, and may even end exactly on a true frame's start - nothing points at it.)
//   k_sp_place    one workgroup: the scan over the reachable LZ4-frame nodes -> d_src_off and the record; the chain's last node gives
//                 the stop: its own status, or srcBytes, or the verdict of sp_step at the position its frame ends on
//   k_split_serial  one thread walks (returns at once unless overflow is flagged or the engine is forced serial), the workgroup fills
// A frame of B blocks costs its node's thread B dependent reads, about 0.35 us each (176 MiB of stream: 0.15 ms as 4096 frames of 2
// blocks, 0.32 ms as 8 frames of 512 blocks): the call is for streams of many frames, not for the one big frame of the single call's
// parallel walks.  The node list's capacity and the rounds: sp_node_cap, sp_rounds (engine.hip); the contract: include/lz4f_mi355x.h.
#pragma once
#include "common.cuh"
#include "batch_common.cuh"

namespace lz4f {

constexpr uint32_t SP_CHUNK = 16384, SP_THREADS = 256, SP_UNITS = SP_CHUNK / 16 / SP_THREADS;      // units per thread and chunk
static_assert(SP_UNITS == 4, "k_sp_list reads a thread's four unit masks as one u64");
constexpr uint32_t SP_NONE = 0xFFFFFFFFu;                // a link to no node
constexpr uint32_t SP_FRAME = 1u << 31, SP_SKIP = 1u << 30;      // SpNode::st: what ended at `end` (neither: the status, and no end)

struct SpCtl {                                           // the call's control block (device workspace, written by k_sp_order first)
    uint32_t overflow;                                   // the parallel kernels do not deliver: k_split_serial does
    uint32_t total;                                      // nodes
};
struct SpNode { uint64_t end; uint32_t st, link; };      // link: the node at `end`, SP_NONE: none (the doubling rounds work on copies)

// The model's step at `pos` < src_bytes: what batch_frame_head says of S[pos .. src_bytes) with no bound on the blocks and no
// per-block predicate -> 0 and consumed > 0 (skippable: it was a skippable frame), or the status the walk stops with
__device__ __forceinline__ uint32_t sp_step(const uint8_t* __restrict__ src, uint64_t src_bytes, uint64_t pos, uint64_t& consumed, bool& skippable)
{
    BatchCore r;
    batch_core_init(r, pos);
    r.span = src_bytes - pos;
    const uint32_t st = batch_frame_head(src, r, [](uint32_t) -> uint64_t { return ~0ull; }, [](uint32_t) -> uint32_t { return ST_OK; });
    consumed = r.consumed;
    skippable = st == ST_OK && (r.flags & FLAG_SKIPPABLE) != 0;              // (a frame's flags are its FLG byte: bit 8 is clear)
    return st;
}

// is `p` (p + 4 <= src_bytes, its word v a magic) a node?
__device__ __forceinline__ bool sp_is_node(const uint8_t* __restrict__ src, uint64_t src_bytes, uint64_t p, uint32_t v)
{
    const uint64_t left = src_bytes - p;
    if (v == FRAME_MAGIC) { FrameHead h; return frame_head_parse(src + p, left, h) == ST_OK; }
    uint64_t c;
    return left >= 8 && skippable_span(src + p, left, c) == ST_OK;
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_cand(const uint8_t* __restrict__ src, uint64_t src_bytes, uint32_t n_chunks,
                                                        uint16_t* __restrict__ bits, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_n;
    // 20 bytes: a thread's 16 positions' words (guarded at the stream's end), as k_walk_cand loads them
    auto load20 = [&](uint64_t p0, uint32_t (&w)[5]) {
        w[0] = w[1] = w[2] = w[3] = w[4] = 0;
        if (p0 >= src_bytes) return;
        if (p0 + 20 <= src_bytes) { const b16_ua t = *(const b16_ua*)(src + p0); w[0] = t.a; w[1] = t.b; w[2] = t.c; w[3] = t.d; w[4] = *(const u32_ua*)(src + p0 + 16); }
        else { for (uint32_t k = 0; k < 20 && p0 + k < src_bytes; k++) w[k >> 2] |= (uint32_t)src[p0 + k] << (8 * (k & 3)); }
    };
    auto scan16 = [&](uint64_t p0, const uint32_t (&w)[5]) -> uint32_t {
        uint32_t mask = p0 == 0 ? 1u : 0u;                                  // the root
        if (p0 + 4 > src_bytes) return mask;
        // every magic's top byte is 0x18: where none of the 16 positions' top bytes (bytes 3..18 of the 20) is, there is nothing to
        // look at.  (SWAR zero-byte test on x ^ 0x18181818; a borrow can only add false alarms.)
        auto zb = [](uint32_t x) { const uint32_t y = x ^ 0x18181818u; return (y - 0x01010101u) & ~y & 0x80808080u; };
        if (((zb(w[0]) & 0x80000000u) | zb(w[1]) | zb(w[2]) | zb(w[3]) | (zb(w[4]) & 0x00808080u)) == 0u) return mask;
        uint32_t magic = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t sh = (i & 3) * 8;
            const uint32_t v = sh ? (w[i >> 2] >> sh) | (w[(i >> 2) + 1] << (32 - sh)) : w[i >> 2];
            magic |= (v == FRAME_MAGIC || is_skippable(v)) ? 1u << i : 0u;
        }
#pragma unroll 1
        while (magic) {                                                     // (rare: a loop, not 16 inlined header parses)
            const uint32_t i = (uint32_t)__builtin_ctz(magic);
            magic &= magic - 1;
            const uint64_t p = p0 + i;
            if (p + 4 > src_bytes) continue;
            if (sp_is_node(src, src_bytes, p, rd32le(src + p))) mask |= 1u << i;
        }
        return mask;
    };
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const uint64_t c0 = (uint64_t)chunk * SP_CHUNK + threadIdx.x * 16u;
        constexpr uint32_t STRIDE = SP_THREADS * 16;
        uint32_t wa[5], wb[5], wc[5], wd[5];
        load20(c0, wa); load20(c0 + STRIDE, wb); load20(c0 + 2 * STRIDE, wc); load20(c0 + 3 * STRIDE, wd);
        const uint32_t ma = scan16(c0, wa), mb = scan16(c0 + STRIDE, wb), mc = scan16(c0 + 2 * STRIDE, wc), md = scan16(c0 + 3 * STRIDE, wd);
        uint16_t* b = bits + (uint64_t)chunk * (SP_CHUNK / 16) + threadIdx.x;
        b[0] = (uint16_t)ma; b[SP_THREADS] = (uint16_t)mb; b[2 * SP_THREADS] = (uint16_t)mc; b[3 * SP_THREADS] = (uint16_t)md;
        const uint32_t n = (uint32_t)(__builtin_popcount(ma) + __builtin_popcount(mb) + __builtin_popcount(mc) + __builtin_popcount(md));
        if (n) atomicAdd(&s_n, n);
        __syncthreads();
        if (threadIdx.x == 0) counts[chunk] = s_n;
        __syncthreads();
    }
}

// counts[c] -> the place of chunk c's first node in the list (in place); ctl: the total, and overflow beyond the list's capacity
__global__ __launch_bounds__(1024) void k_sp_order(uint32_t* __restrict__ counts, uint32_t n_chunks, uint32_t node_cap, SpCtl* __restrict__ ctl)
{
    __shared__ WgScan<1> s;
    wg_scan_begin(s);
    for (uint64_t base = 0; base < n_chunks; base += 1024) {
        const uint64_t c = base + threadIdx.x;
        const uint64_t n[1] = {c < n_chunks ? counts[c] : 0u};
        uint64_t at[1];
        wg_scan_tile(n, at, s);
        if (c < n_chunks) counts[c] = (uint32_t)(at[0] < node_cap ? at[0] : node_cap);
    }
    if (threadIdx.x == 0) {
        const uint64_t total = s.carry[0];
        ctl->overflow = total > node_cap ? 1u : 0u;
        ctl->total = (uint32_t)(total > node_cap ? 0u : total);
    }
}

// a thread takes four consecutive units (64 positions, one u64 of bits); the workgroup's scan orders the chunk's nodes
__global__ __launch_bounds__(SP_THREADS) void k_sp_list(const uint64_t* __restrict__ bits, const uint32_t* __restrict__ chunk_at, uint32_t n_chunks,
                                                        const SpCtl* __restrict__ ctl, uint64_t* __restrict__ list)
{
    __shared__ uint32_t s_w[SP_THREADS / WAVE];
    if (ctl->overflow) return;
    const uint32_t total = ctl->total;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t at0 = chunk_at[chunk], at1 = chunk + 1 < n_chunks ? chunk_at[chunk + 1] : total;
        if (at0 == at1) continue;                                           // (uniform)
        uint64_t m = bits[(uint64_t)chunk * SP_THREADS + threadIdx.x];
        const uint32_t n = (uint32_t)__builtin_popcountll(m);
        const uint32_t incl = dpp_incl_scan_add(n);
        if (lane_id() == WAVE - 1) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t at = at0 + incl - n;
        for (uint32_t q = 0; q < (threadIdx.x >> 6); q++) at += s_w[q];
        const uint64_t p0 = (uint64_t)chunk * SP_CHUNK + threadIdx.x * 64u;
        while (m) {
            const uint32_t i = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            if (at < at1) list[at] = p0 + i;                                // (at < at1 <= total <= the capacity)
            at++;
        }
        __syncthreads();
    }
}

// the node at position p, or SP_NONE: bisection over the sorted list
__device__ __forceinline__ uint32_t sp_find(const uint64_t* __restrict__ list, uint32_t total, uint64_t p)
{
    uint32_t a = 0, b = total;                                              // list[a] <= p < list[b]  (list[0] = 0)
    while (b - a > 1) { const uint32_t mid = a + (b - a) / 2; if (list[mid] <= p) a = mid; else b = mid; }
    return list[a] == p ? a : SP_NONE;
}

__global__ __launch_bounds__(256) void k_sp_extent(const uint8_t* __restrict__ src, uint64_t src_bytes, const SpCtl* __restrict__ ctl,
                                                   const uint64_t* __restrict__ list, SpNode* __restrict__ nodes, uint32_t* __restrict__ jump,
                                                   uint8_t* __restrict__ reach)
{
    if (ctl->overflow) return;
    const uint32_t total = ctl->total;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint64_t pos = list[i];
        SpNode nd; nd.end = pos; nd.st = ST_OK; nd.link = SP_NONE;
        if (pos < src_bytes) {                                              // (the root of an empty stream: the walk is over, OK)
            uint64_t consumed = 0; bool skip = false;
            const uint32_t st = sp_step(src, src_bytes, pos, consumed, skip);
            if (st) nd.st = st;
            else {
                nd.end = pos + consumed; nd.st = skip ? SP_SKIP : SP_FRAME;
                if (nd.end < src_bytes) nd.link = sp_find(list, total, nd.end);
            }
        }
        nodes[i] = nd; jump[i] = nd.link; reach[i] = i == 0 ? 1 : 0;
    }
}

// one round: what is reachable reaches its jump; every jump doubles (jin -> jout)
__global__ __launch_bounds__(256) void k_sp_double(const SpCtl* __restrict__ ctl, const uint32_t* __restrict__ jin, uint32_t* __restrict__ jout,
                                                   uint8_t* reach)
{
    if (ctl->overflow) return;
    const uint32_t total = ctl->total;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t j = jin[i];
        uint32_t jj = SP_NONE;
        if (j < total) { if (reach[i]) reach[j] = 1; jj = jin[j]; }
        jout[i] = jj;
    }
}

// what the walk's end says (one thread) -> the record and the fill value of the surplus offsets
struct SpEnd { uint64_t pos, bytes, cut; uint32_t status, n, skipped; };
__device__ __forceinline__ uint64_t sp_finish(const SpEnd& w, uint32_t max_frames, ResultRec* __restrict__ rec, uint32_t path)
{
    if (rec) {
        ResultRec x;
        x.size = w.bytes; x.consumed = w.pos; x.n_blocks = w.n;
        x.status = w.status ? w.status : (w.n > max_frames ? (uint32_t)ST_DSTSMALL : (uint32_t)ST_OK);
        x.first_bad_block = w.status ? w.n : BF_NONE;
        x.flags = (w.skipped ? FLAG_SKIPPABLE : 0u) | (path << 12);
        *rec = x;
    }
    return w.n > max_frames ? w.cut : w.pos;
}

__global__ __launch_bounds__(1024) void k_sp_place(const uint8_t* __restrict__ src, uint64_t src_bytes, SpCtl* __restrict__ ctl,
                                                   const uint64_t* __restrict__ list, const SpNode* __restrict__ nodes,
                                                   const uint8_t* __restrict__ reach, uint32_t max_frames, uint64_t* __restrict__ off,
                                                   ResultRec* __restrict__ rec)
{
    __shared__ WgScan<2> s;
    __shared__ uint32_t sh_last, sh_skipped, sh_bad;
    __shared__ uint64_t sh_cut, sh_fill;
    if (ctl->overflow) return;
    const uint32_t total = ctl->total;
    if (threadIdx.x == 0) { sh_last = SP_NONE; sh_skipped = 0; sh_cut = 0; sh_bad = 0; }
    wg_scan_begin(s);
    for (uint64_t base = 0; base < total; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < total && reach[i];
        SpNode nd; nd.end = 0; nd.st = 0; nd.link = 0;
        uint64_t pos = 0;
        if (live) { nd = nodes[i]; pos = list[i]; }
        const bool frame = live && (nd.st & SP_FRAME);
        const uint64_t c[2] = {frame ? 1u : 0u, frame ? nd.end - pos : 0u};
        uint64_t at[2];
        wg_scan_tile(c, at, s);
        if (frame && at[0] < max_frames) off[at[0]] = pos;
        if (frame && at[0] == max_frames) sh_cut = pos;
        if (live && (nd.st & SP_SKIP)) sh_skipped = 1;
        if (live && nd.link == SP_NONE) sh_last = (uint32_t)i;                        // (the chain is a path: one reachable node ends it)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        SpEnd w;
        w.n = (uint32_t)s.carry[0]; w.bytes = s.carry[1]; w.cut = sh_cut; w.skipped = sh_skipped; w.status = ST_OK; w.pos = src_bytes;
        const uint32_t last = sh_last;
        if (last == SP_NONE) sh_bad = 1;
        else {
            const SpNode nd = nodes[last];
            if (!(nd.st & (SP_FRAME | SP_SKIP))) { w.status = nd.st; w.pos = list[last]; }      // the node itself stops the walk (or: an empty stream)
            else if (nd.end < src_bytes) {                                                       // it ends on a position that is no node
                uint64_t consumed; bool skip;
                w.pos = nd.end;
                w.status = sp_step(src, src_bytes, nd.end, consumed, skip);
                if (w.status == ST_OK) sh_bad = 1;                                               // (a node the list does not have: never)
            }
        }
        if (sh_bad) ctl->overflow = 1;                                                           // k_split_serial delivers
        else sh_fill = sp_finish(w, max_frames, rec, LZ4F_MI355X_PATH_BATCH | LZ4F_MI355X_PATH_PARALLEL_WALK);
    }
    __syncthreads();
    if (sh_bad) return;
    const uint64_t n = s.carry[0], fill = sh_fill;
    for (uint64_t i = (n < max_frames ? n : max_frames) + threadIdx.x; i <= max_frames; i += 1024) off[i] = fill;
}

// the model, verbatim, by one thread; then the workgroup fills the surplus offsets.  force: the engine skips the parallel kernels
__global__ __launch_bounds__(256) void k_split_serial(const uint8_t* __restrict__ src, uint64_t src_bytes, const SpCtl* __restrict__ ctl, uint32_t force,
                                                      uint32_t max_frames, uint64_t* __restrict__ off, ResultRec* __restrict__ rec)
{
    __shared__ uint64_t sh_fill, sh_n;
    if (!force && !ctl->overflow) return;
    if (threadIdx.x == 0) {
        SpEnd w;
        w.pos = 0; w.bytes = 0; w.cut = 0; w.status = ST_OK; w.n = 0; w.skipped = 0;
        while (w.pos < src_bytes) {
            uint64_t consumed = 0; bool skip = false;
            if (const uint32_t st = sp_step(src, src_bytes, w.pos, consumed, skip)) { w.status = st; break; }
            if (skip) w.skipped = 1;
            else {
                if (w.n < max_frames) off[w.n] = w.pos;
                if (w.n == max_frames) w.cut = w.pos;
                w.n++; w.bytes += consumed;
            }
            w.pos += consumed;
        }
        sh_fill = sp_finish(w, max_frames, rec, LZ4F_MI355X_PATH_BATCH);
        sh_n = w.n;
    }
    __syncthreads();
    const uint64_t n = sh_n, fill = sh_fill;
    for (uint64_t i = (n < max_frames ? n : max_frames) + threadIdx.x; i <= max_frames; i += 256) off[i] = fill;
}

}  // namespace lz4f
