// measure_batch.cuh -- what a batch of frames decodes to, without decoding it (lz4f_mi355x_dev_measureFrames): every frame's
// decoded size from its tokens, the verdict the batch decoder gives without looking at decoded bytes, and the window
// lz4f_mi355x_dev_decompressFrames needs for it.  Nothing is written but the records, the offsets and the engine's workspace.
//
// The batch decoder's shape with no window to bound anything (batch_common.cuh: the scan, the record, the frame head, the walks, the
// slice check and the slice verdict); what is this file's own:
//   k_mf_head    a thread per frame: the span against the buffer, then batch_frame_head with the span's bound alone -> a MeasFrame
//                record and a block count
//   (k_batch_place<MeasFrame> then gives every frame a slice of the block table, linked frames too: a block's size needs no
//                history.  The table holds n_frames + srcBytes / 256 + 1 entries (the host's bound, from the call's arguments
//                alone); a frame behind an overflow - 5 bytes of source can be a whole block - goes to k_mf_serial)
//   k_mf_table   a thread per placed frame writes its entries (batch_table_walk)
//   k_mf_blocks  a wave per entry, striding: mf_measure_block, the lanes finding the tokens (decode_indexed.cuh:
//                k_selfindex_walk_wave) under the DECODER's end-of-block rules (decode.cuh: wave_decode_block_lim) judged against
//                room = maxBlockSize.  The two offset bytes of a match are stepped over, never looked at; nothing is hashed
//   k_mf_serial  a wave per frame without a slice: its blocks in order through the same routine
//   k_mf_finish  a wave per frame: first failure, sum, the window, the content-size verdict, the record
//   k_mf_scan    one workgroup: exclusive scan of the windows -> d_dst_off (only when the caller asked for it)
//
// THE WINDOW.  What dev_decompressFrames needs for a frame of n blocks of maxBlockSize bs, block b decoding to got[b], read off
// its kernels:
//   - k_bf_head rejects a frame (linked or not) unless every block's provisional place lies inside the window: b * bs < win for
//     every b, so win >= (n - 1) * bs + 1;
//   - k_bf_table / k_bf_serial give block b of an independent frame the room min(win - b * bs, bs) at b * bs, and it must hold
//     got[b]: for b < n - 1 the first rule already leaves a whole block, for the last one win >= (n - 1) * bs + got[n - 1];
//   - k_bf_serial gives block b of a linked frame the room min(win - out, bs) at out = got[0] + .. + got[b - 1] <= b * bs: again a
//     whole block for b < n - 1 by the first rule, and win >= size for the last one;
//   - the tight last block: a last block with less than a whole block of room that does not decode in it is judged again against
//     a whole block and written if it fits (k_bf_finish / k_bf_serial: bf_redo_tight) whenever win % bs != 0.  For the windows
//     below win % bs == 0 only when the last block has a whole block of room anyway.
// So W = 0 for no blocks, (n - 1) * bs + max(got[n - 1], 1) for independent blocks and max(size, (n - 1) * bs + 1) for linked
// ones: W == size when every block but the last decodes to bs and the last one to something, and W <= n * bs always.
#pragma once
#include "common.cuh"
#include "batch_common.cuh"
#include "lz4_seq.cuh"

namespace lz4f {

constexpr uint32_t MF_SHARE = 256;          // table entries: n_frames + srcBytes / MF_SHARE + 1

using MeasFrame = BatchCore;                // per frame (64 bytes).  tbl_at == BF_NONE: k_mf_serial measures it, and leaves what the last block decodes to in `last`
struct MeasBlk {                            // block table entry (24 bytes)
    uint64_t src;                           // payload in d_src
    uint32_t word, frame;                   // size word, frame
    int32_t got, pad;                       // decoded bytes; -1 malformed
};

// What one compressed block decodes to, by one wave, with no output: -1 where wave_decode_block_lim(in, csize, ., room, ., hist)
// returns -1 for a reason other than a match's offset.  readable: bytes that may be read from `in` on (the span's end), >= csize.
__device__ __forceinline__ int32_t mf_measure_block(const uint8_t* __restrict__ in, uint32_t csize, uint64_t readable, uint32_t room)
{
    if (csize == 0) return -1;
    const uint32_t lane = lane_id();
    uint32_t pos = 0, op = 0;                                    // (op <= room throughout)
    for (;;) {
        if (pos >= csize) return -1;                              // a token is due and the payload is over
        // ---- the lanes' path (wave_decode_block_win's condition: none of a window's sequences can be the block's last or come near room) ----
        if (csize - pos >= 96u && room - op >= 1024u) {
            const uint32_t d = *(const u32_ua*)(in + pos + lane);
            const LaneTok tk = lane_token(d);
            const uint32_t hdr = tk.hdr, lit = tk.lit, ml = tk.ml;
            const bool easy = ml != 15u && !(hdr == 2u && tk.e1 == 255u) && lane + hdr + lit + 2u <= 64u;
            uint32_t s;
            const uint64_t mask = hop_tokens(easy ? lane + hdr + lit + 2u : 255u, s);
            if (mask) {
                const bool is_tok = (mask >> lane) & 1ull;
                const uint32_t incl = dpp_incl_scan_add(is_tok ? lit + ml + 4u : 0u);
                op += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);         // (<= 442: still >= 582 below room)
                pos += s;
                continue;
            }
        }
        // ---- one sequence, wave-uniformly, under the decoder's rules ----
        SeqCur c{pos, 0};                                         // (no carried window: the next step may be the lanes')
        seq_begin(in, readable, c);
        c.w = uni64(c.w);
        uint32_t token, lit, p, mlen;
        if (!seq_lit<true>(in, csize, c, token, lit, p) || p > csize || lit > (1u << 24)) return -1;     // (a length byte beyond the payload; more literals than any payload has)
        const uint32_t in_left = csize - p, out_left = room - op;
        if (lit + 12 > out_left || lit + 8 > in_left) {           // must be the last sequence: its literals end exactly at the payload's end
            if (lit != in_left || lit > out_left) return -1;
            return (int32_t)(op + lit);
        }
        op += lit;
        const uint32_t q = p + lit;                               // the offset's two bytes: stepped over
        uint64_t w2 = 0, w2_hi = 0;
        if ((token & 15) == 15) { pt_load16(in, q, readable, w2, w2_hi); w2 = uni64(w2); }
        if (!seq_match<true>(in, csize, readable, c, token, q, w2, w2_hi, mlen)) return -1;
        if ((token & 15) == 15 && c.pos + 4 >= csize) return -1;          // length bytes stop before iend - 4
        mlen += 4;
        if ((uint64_t)mlen + 5 > (uint64_t)(room - op)) return -1;    // the last 5 bytes must be literals
        op += mlen;
        pos = c.pos;
    }
}
__device__ __forceinline__ int32_t mf_measure_word(const uint8_t* __restrict__ in, uint32_t word, uint64_t readable, uint32_t room)
{
    const uint32_t csz = word_size(word);
    return word_stored(word) ? (int32_t)csz : mf_measure_block(in, csz, readable, room);       // (csz <= maxBlockSize: the walk)
}

__global__ __launch_bounds__(256) void k_mf_head(const uint8_t* __restrict__ src, uint64_t src_bytes, const uint64_t* __restrict__ soff, uint32_t n_frames,
                                                 MeasFrame* __restrict__ frames, uint32_t* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    MeasFrame r;
    batch_core_init(r, soff[i]);
    const uint64_t s1 = soff[i + 1];
    uint32_t count = 0;
    auto put = [&](uint32_t st) { r.status = st; frames[i] = r; counts[i] = count; };
    if (r.src > s1 || s1 > src_bytes) { r.src = 0; return put(ST_SRCPTR); }                 // nothing is read
    const uint64_t cap = r.span = s1 - r.src;
    // k_bf_head's bound on the blocks of a span, the part of it that no window changes: more size words than a block per 5 bytes
    // of span (only empty stored blocks, 4 bytes each, get there) is dstMaxSize_tooSmall to the decoder in any window, so here too
    const uint32_t st = batch_frame_head(src, r, [&](uint32_t) { return cap / 5 + 2; }, [](uint32_t) -> uint32_t { return ST_OK; });
    if (st == ST_OK) count = r.n_blocks;
    put(st);
}

__global__ __launch_bounds__(256) void k_mf_table(const uint8_t* __restrict__ src, const MeasFrame* __restrict__ frames, uint32_t n_frames,
                                                  MeasBlk* __restrict__ table)
{
    batch_table_walk(src, frames, n_frames, [&](uint32_t i, const MeasFrame& r, uint32_t b, uint32_t w, uint64_t at) {
        MeasBlk e;
        e.src = r.src + at; e.word = w; e.frame = i; e.got = 0; e.pad = 0;
        table[r.tbl_at + b] = e;
    });
}

// the grid is sized by the host's bound on the table, capped: the waves stride over the entries in use (ctl[0])
template <int W>
__global__ __launch_bounds__(64 * W) void k_mf_blocks(const uint8_t* __restrict__ src, const MeasFrame* __restrict__ frames, uint32_t n_frames,
                                                      MeasBlk* __restrict__ table, const uint32_t* __restrict__ ctl)
{
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t total = uni(ctl[0]);
    for (uint32_t w = uni(blockIdx.x * W + wv); w < total; w += gridDim.x * W) {
        const MeasBlk e = table[w];
        const uint32_t fi = uni(e.frame);
        if (fi >= n_frames) continue;
        if (!slice_holds(uni(frames[fi].tbl_at), uni(frames[fi].n_blocks), w)) continue;
        const uint64_t span_end = uni64(frames[fi].src + frames[fi].span);
        const uint64_t so = uni64(e.src);
        const int32_t got = mf_measure_word(src + so, uni(e.word), span_end - so, uni(frames[fi].bs));
        if (lane_id() == 0) table[w].got = got;
    }
}

// a wave per frame without a table slice: blocks in order, the same routine
template <int W>
__global__ __launch_bounds__(64 * W) void k_mf_serial(const uint8_t* __restrict__ src, MeasFrame* __restrict__ frames, uint32_t n_frames)
{
    const uint32_t i = uni(blockIdx.x * W + (threadIdx.x >> 6));
    if (i >= n_frames) return;
    const uint32_t status = uni(frames[i].status), n = uni(frames[i].n_blocks), tbl_at = uni(frames[i].tbl_at);
    if (status != 0 || n == 0 || tbl_at != BF_NONE) return;
    const uint64_t s0 = uni64(frames[i].src), span = uni64(frames[i].span);
    const uint32_t flg = uni(frames[i].flags), bs = uni(frames[i].bs);
    const uint8_t* f = src + s0;
    uint64_t pos = uni(frames[i].hsize), out = 0;
    uint32_t b, last = 0;
    // (k_mf_head has held every word of this frame to its span: no bound to hold them to again)
    const uint32_t st = bf_walk<true>(f, ~0ull, pos, b, bs, flg_bck(flg), [&](uint32_t word, uint32_t, uint64_t src_at) -> uint32_t {
        const int32_t got = mf_measure_word(f + src_at, word, span - src_at, bs);
        if (got < 0) return ST_GENERIC;
        last = (uint32_t)got;
        out += last;
        return ST_OK;
    });
    if (lane_id() == 0) {
        if (st) { frames[i].status = st; frames[i].first_bad = b; }
        else { frames[i].status = frame_size_status(flg, frames[i].size, out); frames[i].size = out; frames[i].last = last; }
    }
}

template <int W>
__global__ __launch_bounds__(64 * W) void k_mf_finish(const MeasFrame* __restrict__ frames, uint32_t n_frames, const MeasBlk* __restrict__ table,
                                                      ResultRec* __restrict__ results, uint64_t* __restrict__ wins)
{
    const uint32_t i = uni(blockIdx.x * W + (threadIdx.x >> 6));
    if (i >= n_frames) return;
    const uint32_t lane = lane_id();
    const MeasFrame r = frames[i];
    uint32_t status = uni(r.status), first_bad = uni(r.first_bad), last = uni(r.last);
    uint64_t size = uni64(r.size);
    const uint32_t n = uni(r.n_blocks), flg = uni(r.flags), bs = uni(r.bs), tbl_at = uni(r.tbl_at);
    if (status == 0 && n == 0) {                                   // no blocks: an empty frame, or a skippable one
        status = frame_size_status(flg, size, 0);
        size = 0;
    } else if (status == 0 && tbl_at != BF_NONE) {                 // the placed frames: the verdict on the table slice
        const MeasBlk* t = table + tbl_at;
        uint32_t bad; int32_t kind; uint64_t sum;
        slice_verdict(n, bad, kind, sum, [&](uint32_t b) -> int32_t { return b < n ? t[b].got : 0; });
        if (bad != BF_NONE) { status = ST_GENERIC; first_bad = bad; }
        else {
            last = uni((uint32_t)t[n - 1].got);
            status = frame_size_status(flg, size, sum);
            size = sum;
        }
    }
    // the window (the rule and where it comes from: the head of this file)
    uint64_t win = 0;
    if (status == 0 && n) {
        const uint64_t places = (uint64_t)(n - 1) * bs;
        win = flg_indep(flg) ? places + (last ? last : 1u) : (size > places + 1 ? size : places + 1);
    }
    if (status != 0 && status != ST_FRAMESIZE) size = 0;             // (nothing measured to the end)
    if (lane == 0) {
        ResultRec x;
        x.size = size; x.consumed = uni64(r.consumed); x.status = status; x.n_blocks = n; x.first_bad_block = first_bad;
        x.flags = (flg & 0xFFFu) | (LZ4F_MI355X_PATH_BATCH << 12);
        results[i] = x;
        wins[i] = win;
    }
}

// one workgroup: off[i] = wins[0] + .. + wins[i - 1], off[n_frames] the total
__global__ __launch_bounds__(1024) void k_mf_scan(const uint64_t* __restrict__ wins, uint32_t n_frames, uint64_t* __restrict__ off)
{
    __shared__ WgScan<1> s;
    wg_scan_begin(s);
    for (uint32_t base = 0; base < n_frames; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t c[1] = {i < n_frames ? wins[i] : 0u};
        uint64_t at[1];
        wg_scan_tile(c, at, s);
        if (i < n_frames) off[i] = at[0];
    }
    if (threadIdx.x == 0) off[n_frames] = s.carry[0];
}

}  // namespace lz4f
