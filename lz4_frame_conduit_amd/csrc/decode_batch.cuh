// decode_batch.cuh -- many independent frames in one call (lz4f_mi355x_dev_decompressFrames), no host read in between.
//
// The single-frame call reads the header back to the host to pick its plan; here every frame carries its own plan on the
// device, and every kernel takes all frames at once.  The scan, the record's core, the frame head, the walks, the slice check and
// the slice verdict are batch_common.cuh's; what is this file's own:
//   k_bf_head    a thread per frame: the span and the window checked against the buffers, then batch_frame_head held to the window
//                (every block's provisional place, b * maxBlockSize, inside it) -> a BatchFrame record and a block count
//   (k_batch_place<BatchFrame> then gives the independent frames their slices of the block table.  The host sizes the table
//                n_frames + dstBytes / 64 KiB + 1, so the workspace needs no read-back.  A walked frame has n_blocks <=
//                window / 64 KiB + 1, so frames whose windows do not overlap always fit; only windows that overlap can overflow
//                the table, and a frame behind the overflow is decoded by k_bf_serial instead - it still decodes as it would alone)
//   k_bf_table   a thread per placed frame writes its entries (batch_table_walk)
//   k_bf_blocks  a wave per entry: block checksum, then the block decoded as k_decode_blocks does (wave_decode_block_win), its
//                readable bound the frame's span end
//   k_bf_serial  a wave per frame that has no table slice (linked frames; independent frames behind a table overflow): checksums
//                and blocks in order, history from the frame's own window; the verdict as k_finish_decode gives it
//   k_bf_finish  a wave per frame: the placed frames' verdict (tight last block, first failure, packing, content size), then
//                every frame's content checksum - the chains of different frames run side by side - and the result record
// Nothing is written outside a frame's window on its behalf: every decode is bounded by the block's room inside the window, and
// the one decode that is judged against a whole block (the tight last block, k_redo_tight_block's rule) only writes what fits.
//
// THE SHARED DICTIONARY (lz4f_mi355x_dev_decompressFrames_usingDict).  One dictionary for the whole batch: the history in front of a
// frame's output (linked blocks), or in front of every block (independent blocks), is the dictionary's last <= 64 KiB, as
// LZ4F_decompress_usingDict has it.  The three kernels that decode blocks are templates, k_bf_blocks / k_bf_serial / k_bf_finish
// <W, DICT>, and take the dictionary by value (DictTail, common.cuh: the type the batch encoder's EncDict begins with).  With DICT set
// (these instantiations were k_bf_blocks_dict, k_bf_serial_dict, k_bf_finish_dict) every block goes through the scalar-parse decoder
// (wave_decode_block_lim<true, true>: the offset check and the two-part match copy are there, decode.cuh) - independent blocks too,
// which the plain call gives to wave_decode_block_win.  The plain call launches the DICT = false instantiations, which ignore `dc`.
//
// A SET OF DICTIONARIES (lz4f_mi355x_dev_decompressFrames_usingDictSet, dictset.cuh).  The dictionary is the frame's, not the call's:
// k_bf_head<true> resolves every frame's slot - the caller's, or what the header's dictID names - into an array beside the frame
// records (4 bytes a frame, this call's own workspace), and the third form of the three kernels, <W, BF_SET>, takes the set's table
// and that array (BfSet) where the others take `dc`: the wave loads its frame's DictTail from the table, wave-uniform.  A frame
// with a member of at least one byte decodes as DICT = true decodes it, every other frame as DICT = false does (k_bf_blocks<W, BF_SET>
// has both decoders, and the plain one's LDS), so a frame's bytes and record are what the one-dictionary calls give it alone.
#pragma once
#include "common.cuh"
#include "decode.cuh"
#include "batch_common.cuh"
#include "dictset.cuh"
#include <type_traits>

namespace lz4f {

constexpr uint32_t BF_SHARE = 65536;       // table entries per frame: window / BF_SHARE + 1

struct BatchFrame : BatchCore {             // per frame (device workspace, 80 bytes); tbl_at == BF_NONE: k_bf_serial decodes it
    uint64_t dst, win;                      // its window in d_dst
};
struct BatchBlk {                           // block table entry (40 bytes)
    uint64_t src, dst;                      // payload in d_src, block's place in d_dst (block b of its frame at b * maxBlockSize)
    uint32_t word, room, frame, ck;         // size word, bytes of the window from dst on (<= maxBlockSize), frame, checksum failed
    int32_t got, pad;                       // decoded bytes; -1 malformed, -2 does not fit
};

// The three forms of the kernels that decode blocks (their template argument DICT; false and true are the first two): no dictionary,
// the call's one dictionary, and BF_SET - a set of dictionaries, each frame with the member its slot names
constexpr int BF_SET = 2;
// what a BF_SET kernel takes where the others take the call's DictTail: the set's table and the frames' resolved slots (k_bf_head<true>)
struct BfSet : DsView {
    const uint32_t* slot = nullptr;
};
template <int DICT> using BfDict = typename std::conditional<DICT == BF_SET, BfSet, DictTail>::type;
// frame fi's dictionary (wave-uniform): the call's, or with BF_SET its member's bytes - none for DS_NONE and for a frame that failed
__device__ __forceinline__ const DictTail& bf_frame_dict(const DictTail& dc, uint32_t) { return dc; }
__device__ __forceinline__ DictTail bf_frame_dict(const BfSet& set, uint32_t fi) { return ds_tail(set, uni(set.slot[fi])); }

// wave_decode_block judged by `cap`, writing only the first `wlim` bytes (decode.cuh: wave_decode_block_lim): -1 malformed, -2
// decodes but not into wlim.  DICT: dc, the batch's dictionary (DictTail, common.cuh), lies in front of the history.  BF_SET: dc is
// the frame's own, and a frame that has none (dc.len 0) decodes as the plain form decodes it
template <int DICT>
__device__ __forceinline__ int32_t bf_decode_block(const uint8_t* __restrict__ in, uint32_t csize, uint8_t* out, uint32_t cap, uint32_t wlim,
                                                   uint64_t hist, const DictTail& dc)
{
    if constexpr (DICT == BF_SET) {                // (both decoders in one kernel: the plain one's cursors need the readfirstlane too)
        if (dc.len) return bf_decode_block<1>(in, csize, out, cap, wlim, hist, dc);
        return wave_decode_block_lim<true, false, true>(in, csize, out, cap, wlim, hist);
    }
    else if constexpr (DICT) return wave_decode_block_lim<true, true>(in, csize, out, cap, wlim, hist, (const uint8_t*)uni64((uint64_t)dc.end), uni(dc.len));
    else return wave_decode_block_lim<true>(in, csize, out, cap, wlim, hist);
}

// dst[0..len) = src[0..len) with dst < src (a block of an independent frame moved down to where the blocks in front of it end)
__device__ __forceinline__ void bf_move_down(uint8_t* dst, const uint8_t* src, uint64_t len)
{
    const uint32_t lane = lane_id();
    uint64_t o = 0;
    for (; o + 1024 <= len; o += 1024) {                    // (a step reads 1 KiB above everything it and the steps before wrote)
        const b16_ua v = *(const b16_ua*)(src + o + lane * 16);
        *(b16_ua*)(dst + o + lane * 16) = v;
    }
    for (; o < len; o += WAVE) {
        uint8_t v = 0;
        if (o + lane < len) v = src[o + lane];
        if (o + lane < len) dst[o + lane] = v;
    }
}

// the tight last block (k_redo_tight_block): judged against a whole block, written only if it fits.  -> size, -2 or -3
template <int DICT>
__device__ __forceinline__ int32_t bf_redo_tight(const uint8_t* in, uint32_t csz, uint8_t* out, uint32_t bs, uint32_t room, uint64_t hist,
                                                 const DictTail& dc)
{
    const int32_t g = bf_decode_block<DICT>(in, csz, out, bs, room, hist, dc);
    return g == -1 ? -3 : g;
}

// SET (k_bf_head<true>): the frame's slot is resolved here and kept in slot[i] for the kernels behind - `given`[i] held to the set, or
// with given == NULL what the header's dictID names.  The verdicts in order: the offsets, the header's own errors, then the slot - a
// slot that is no member fails the frame (ST_GENERIC, an empty record, DS_UNKNOWN in slot[i]: k_bf_finish marks the record) before
// anything of it is walked
// (One kernel template, the set's arguments an empty struct in the plain form: as a shared body behind two kernels the plain form's
// code came out with an add's operands swapped.)
template <bool SET> struct BfHeadSet {};
template <> struct BfHeadSet<true> { DsView set; const uint32_t* given; uint32_t* slot; };
template <bool SET>
__global__ __launch_bounds__(256) void k_bf_head(const uint8_t* __restrict__ src, uint64_t src_bytes, const uint64_t* __restrict__ soff,
                                                 uint64_t dst_bytes, const uint64_t* __restrict__ doff, uint32_t n_frames,
                                                 BatchFrame* __restrict__ frames, uint32_t* __restrict__ counts, BfHeadSet<SET> hs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    BatchFrame r;
    batch_core_init(r, soff[i]);
    r.dst = doff[i]; r.win = 0;
    const uint64_t s1 = soff[i + 1], d1 = doff[i + 1];
    uint32_t count = 0, my_slot = DS_NONE;
    auto put = [&](uint32_t st) {
        r.status = st; frames[i] = r; counts[i] = count;
        if constexpr (SET) hs.slot[i] = my_slot;
    };
    if (r.src > s1 || s1 > src_bytes) { r.src = 0; r.dst = 0; return put(ST_SRCPTR); }      // nothing is read or written
    if (r.dst > d1 || d1 > dst_bytes) { r.src = 0; r.dst = 0; return put(ST_DSTSMALL); }
    r.span = s1 - r.src; r.win = d1 - r.dst;
    const uint64_t cap = r.span, win = r.win;
    if constexpr (SET) {
        bool head_ok;
        my_slot = ds_header_slot(src + r.src, cap, hs.set, head_ok);
        if (hs.given) my_slot = head_ok ? ds_given_slot(hs.given[i], hs.set.count) : DS_NONE;
        if (my_slot == DS_UNKNOWN) return put(ST_GENERIC);
    }
    uint64_t out = 0;
    const uint32_t st = batch_frame_head(src, r,
        [&](uint32_t bs) { const uint64_t by_dst = win / bs + 2, by_src = cap / 5 + 2; return by_src < by_dst ? by_src : by_dst; },    // the single call's table bound
        [&](uint32_t bs) -> uint32_t {
            if (out >= win) return ST_DSTSMALL;
            out += bs;
            return ST_OK;
        });
    if (st == ST_OK && flg_indep(r.flags)) count = r.n_blocks;                          // (<= win / BF_SHARE + 1: out < win held for every block)
    put(st);
}

__global__ __launch_bounds__(256) void k_bf_table(const uint8_t* __restrict__ src, const BatchFrame* __restrict__ frames, uint32_t n_frames,
                                                  BatchBlk* __restrict__ table)
{
    batch_table_walk(src, frames, n_frames, [&](uint32_t i, const BatchFrame& r, uint32_t b, uint32_t w, uint64_t at) {
        const uint64_t out = (uint64_t)b * r.bs;
        BatchBlk e;
        e.src = r.src + at; e.dst = r.dst + out; e.word = w;
        e.room = (uint32_t)(r.win - out < r.bs ? r.win - out : r.bs);
        e.frame = i; e.ck = 0; e.got = 0; e.pad = 0;
        table[r.tbl_at + b] = e;
    });
}

// the grid is sized by the host's bound on the table, capped (engine.hip: BATCH_GRID): the waves stride over the entries in
// use (ctl[0]), so a small batch into a big destination buffer does not launch a workgroup per 64 KiB of it
template <int W, int DICT>
__device__ __forceinline__ void bf_blocks_body(const uint8_t* __restrict__ src, uint8_t* dst, const BatchFrame* __restrict__ frames,
                                               uint32_t n_frames, BatchBlk* __restrict__ table, const uint32_t* __restrict__ ctl,
                                               uint32_t (*expand)[64], const BfDict<DICT>& dc)
{
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t total = uni(ctl[0]);
    for (uint32_t w = uni(blockIdx.x * W + wv); w < total; w += gridDim.x * W) {
        const BatchBlk e = table[w];
        const uint32_t fi = uni(e.frame);
        if (fi >= n_frames) continue;
        if (!slice_holds(uni(frames[fi].tbl_at), uni(frames[fi].n_blocks), w)) continue;
        const uint64_t span_end = uni64(frames[fi].src + frames[fi].span);
        const uint32_t flg = uni(frames[fi].flags);
        const uint64_t so = uni64(e.src), dof = uni64(e.dst);
        const uint32_t word = uni(e.word), room = uni(e.room), csz = word_size(word);
        uint32_t ck = 0;
        if (flg_bck(flg)) {
            const uint32_t h = wave_xxh32(src + so, csz);
            ck = h != rd32le(src + so + csz) ? 1u : 0u;
        }
        int32_t got;
        if (word_stored(word)) {
            if (csz > room) got = -2;
            else { wave_copy_disjoint(dst + dof, src + so, csz); got = (int32_t)csz; }
        } else if constexpr (DICT == BF_SET) {                     // the frame's own member; a frame without one: as the plain form
            const DictTail fd = bf_frame_dict(dc, fi);
            if (fd.len) got = bf_decode_block<1>(src + so, csz, dst + dof, room, room, 0, fd);
            else got = wave_decode_block_win<true>(src + so, csz, span_end - so, dst + dof, room, expand[wv]);
        } else if constexpr (DICT) {
            got = bf_decode_block<true>(src + so, csz, dst + dof, room, room, 0, dc);
        } else {
            got = wave_decode_block_win<true>(src + so, csz, span_end - so, dst + dof, room, expand[wv]);
        }
        if (lane_id() == 0) { table[w].got = got; table[w].ck = ck; }
    }
}
template <int W, int DICT>
__global__ __launch_bounds__(64 * W, 8) void k_bf_blocks(const uint8_t* __restrict__ src, uint8_t* dst, const BatchFrame* __restrict__ frames,
                                                        uint32_t n_frames, BatchBlk* __restrict__ table, const uint32_t* __restrict__ ctl, BfDict<DICT> dc)
{
    if constexpr (DICT == BF_SET) {
        __shared__ uint32_t expand[W][64];                             // (for the frames that have no dictionary)
        bf_blocks_body<W, BF_SET>(src, dst, frames, n_frames, table, ctl, expand, dc);
    } else if constexpr (DICT) bf_blocks_body<W, true>(src, dst, frames, n_frames, table, ctl, nullptr, dc);
    else {
        __shared__ uint32_t expand[W][64];                             // (wave_decode_block_win's: with DICT the kernel has no LDS)
        bf_blocks_body<W, false>(src, dst, frames, n_frames, table, ctl, expand, dc);
    }
}

// a wave per frame without a table slice: blocks in order
template <int W, int DICT>
__device__ __forceinline__ void bf_serial_body(const uint8_t* __restrict__ src, uint8_t* dst, BatchFrame* __restrict__ frames, uint32_t n_frames,
                                               const BfDict<DICT>& dcs)
{
    const uint32_t i = uni(blockIdx.x * W + (threadIdx.x >> 6));
    if (i >= n_frames) return;
    const uint32_t status = uni(frames[i].status), n = uni(frames[i].n_blocks), tbl_at = uni(frames[i].tbl_at);
    if (status != 0 || n == 0 || tbl_at != BF_NONE) return;
    const auto& dc = bf_frame_dict(dcs, i);
    const uint64_t s0 = uni64(frames[i].src), d0 = uni64(frames[i].dst), win = uni64(frames[i].win);
    const uint32_t flg = uni(frames[i].flags), bs = uni(frames[i].bs), bck = flg_bck(flg);
    const bool linked = !flg_indep(flg);
    const uint8_t* f = src + s0;
    uint8_t* o = dst + d0;
    uint64_t pos = uni(frames[i].hsize), out = 0;
    uint32_t b;
    // (k_bf_head has held every word of this frame to its span: no bound to hold them to again)
    const uint32_t st = bf_walk<true>(f, ~0ull, pos, b, bs, bck, [&](uint32_t word, uint32_t csz, uint64_t src_at) -> uint32_t {
        const uint8_t* in = f + src_at;
        if (bck && wave_xxh32(in, csz) != rd32le(in + csz)) return ST_BLOCKCK;               // (the first failure of either kind decides)
        const uint64_t at = linked ? out : (uint64_t)b * bs;                                 // (independent: the provisional place, < win by the walk)
        const uint32_t room = (uint32_t)(win - at < bs ? win - at : bs);
        int32_t got;
        if (word_stored(word)) {
            if (csz > room) got = -2;
            else { wave_copy_disjoint(o + at, in, csz); got = (int32_t)csz; }
        } else {
            got = bf_decode_block<DICT>(in, csz, o + at, room, room, linked ? at : 0, dc);
            if (got < 0 && b + 1 == n && csz && win % bs != 0 && win - at < bs)
                got = bf_redo_tight<DICT>(in, csz, o + at, bs, room, linked ? at : 0, dc);
        }
        if (got < 0) return block_fail_status(got, at, win, bs);
        if (at != out) bf_move_down(o + out, o + at, (uint32_t)got);
        out += (uint32_t)got;
        return ST_OK;
    });
    if (lane_id() == 0) {
        if (st) { frames[i].status = st; frames[i].first_bad = b; }
        else {
            frames[i].status = frame_size_status(flg, frames[i].size, out);
            frames[i].size = out;
        }
    }
}
template <int W, int DICT>        // (DICT: held to 8 waves a SIMD, as the plain form is, the two-part copy spills to scratch: 6 it is)
__global__ __launch_bounds__(64 * W, DICT ? 4 : 8) void k_bf_serial(const uint8_t* __restrict__ src, uint8_t* dst, BatchFrame* __restrict__ frames,
                                                                   uint32_t n_frames, BfDict<DICT> dc)
{
    bf_serial_body<W, DICT>(src, dst, frames, n_frames, dc);
}

template <int W, int DICT>
__device__ __forceinline__ void bf_finish_body(const uint8_t* __restrict__ src, uint8_t* dst, BatchFrame* __restrict__ frames, uint32_t n_frames,
                                               const BatchBlk* __restrict__ table, ResultRec* __restrict__ results, uint32_t content_check,
                                               uint32_t (*park)[XXH_PARK / 4], const BfDict<DICT>& dcs)
{
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t i = uni(blockIdx.x * W + wv);
    if (i >= n_frames) return;
    const auto& dc = bf_frame_dict(dcs, i);
    const uint32_t lane = lane_id();
    const BatchFrame r = frames[i];
    uint32_t status = uni(r.status), first_bad = uni(r.first_bad);
    uint64_t size = uni64(r.size);
    const uint32_t n = uni(r.n_blocks), flg = uni(r.flags), bs = uni(r.bs), tbl_at = uni(r.tbl_at);
    const uint64_t win = uni64(r.win);
    uint8_t* o = dst + uni64(r.dst);
    if (status == 0 && n == 0) {                                   // no blocks: an empty frame, or a skippable one
        status = frame_size_status(flg, size, 0);
        size = 0;
    } else if (status == 0 && tbl_at != BF_NONE) {                 // the placed frames: k_finish_decode's verdict on the table slice
        const BatchBlk* t = table + tbl_at;
        // the tight last block first, as k_redo_tight_block runs before the verdict
        int32_t last = t[n - 1].got;
        const uint64_t last_at = (uint64_t)(n - 1) * bs;
        const uint32_t lw = uni(t[n - 1].word), lcsz = word_size(lw);
        if (uni((uint32_t)last) >> 31 && !word_stored(lw) && lcsz && win % bs != 0 && win - last_at < bs)
            last = bf_redo_tight<DICT>(src + uni64(t[n - 1].src), lcsz, o + last_at, bs, uni(t[n - 1].room), 0, dc);
        last = (int32_t)uni((uint32_t)last);
        uint32_t bad, ck = BF_NONE; int32_t kind; bool moves = false; uint64_t sum;
        slice_verdict(n, bad, kind, sum, [&](uint32_t b) -> int32_t {
            const bool in = b < n;
            const int32_t g = !in ? 0 : b + 1 == n ? last : t[b].got;
            const uint64_t cm = __ballot(in && t[b].ck);
            if (cm && ck == BF_NONE) ck = b - lane + (uint32_t)__builtin_ctzll(cm);
            if (__ballot(in && b + 1 < n && g != (int32_t)bs)) moves = true;
            return g;
        });
        if (ck != BF_NONE && ck <= bad) { status = ST_BLOCKCK; first_bad = ck; }
        else if (bad != BF_NONE) { status = block_fail_status(kind, (uint64_t)bad * bs, win, bs); first_bad = bad; }
        else {
            if (moves) {                                           // a non-final block decoded short: pack the blocks (rare)
                uint64_t out = 0;
                for (uint32_t b = 0; b < n; b++) {
                    const uint32_t g = uni(b + 1 == n ? (uint32_t)last : (uint32_t)t[b].got);
                    const uint64_t at = (uint64_t)b * bs;
                    if (at != out) bf_move_down(o + out, o + at, g);
                    out += g;
                }
            }
            status = frame_size_status(flg, size, sum);
            size = sum;
        }
    }
    // the content checksum, behind the frame's EndMark (k_xxh32_content)
    const uint64_t consumed = uni64(r.consumed);
    if (status == 0 && flg_cck(flg) && !(flg & FLAG_SKIPPABLE) && content_check) {
        const uint32_t h = lane4_xxh32(o, size, park[wv]);
        if (h != rd32le(src + r.src + consumed - 4)) status = ST_CONTENTCK;
    }
    if (lane == 0) {
        ResultRec x;
        x.size = size; x.consumed = consumed; x.status = status; x.n_blocks = n; x.first_bad_block = first_bad;
        x.flags = (flg & 0xFFFu) | (LZ4F_MI355X_PATH_BATCH << 12);
        if constexpr (DICT == BF_SET) { if (dcs.slot[i] == DS_UNKNOWN) x.flags |= LZ4F_MI355X_PATH_DICT_UNKNOWN << 12; }
        results[i] = x;
    }
}
template <int W, int DICT>
__global__ __launch_bounds__(64 * W) void k_bf_finish(const uint8_t* __restrict__ src, uint8_t* dst, BatchFrame* __restrict__ frames, uint32_t n_frames,
                                                      const BatchBlk* __restrict__ table, ResultRec* __restrict__ results, uint32_t content_check,
                                                      BfDict<DICT> dc)
{
    __shared__ __attribute__((aligned(16))) uint32_t park[W][XXH_PARK / 4];
    bf_finish_body<W, DICT>(src, dst, frames, n_frames, table, results, content_check, park, dc);
}

}  // namespace lz4f
