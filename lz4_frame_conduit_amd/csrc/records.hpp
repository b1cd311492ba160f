// records.hpp -- the records and codes the kernels and the host-pointer layer share.  Plain C++: no device code, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lz4f_mi355x.h"
#include "frame_format.hpp"      // the status codes the kernels write, and the frame grammar

namespace lz4f {

// ---- records shared with the host (include/lz4f_mi355x.h) ----
struct BlockOut {            // mirrors lz4f_mi355x_block
    uint64_t src_off, dst_off;
    uint32_t word, dst_size;
};
struct ResultRec {           // mirrors lz4f_mi355x_result
    uint64_t size, consumed;
    uint32_t status, n_blocks, first_bad_block, flags;
};
static_assert(sizeof(BlockOut) == sizeof(lz4f_mi355x_block), "block table layout");
static_assert(sizeof(ResultRec) == sizeof(lz4f_mi355x_result), "result layout");

// ---- the trailer behind a frame (frame_dev.cuh: the trailer; the host writes the same bytes for frames it assembles) ----
constexpr uint32_t TR_MAGIC = SKIP_MAGIC | 0xEu, TR_FOOT = 0x58495A4Cu;
struct TrailerFoot { uint32_t total_seqs, total_entries, pad0, pad1, magic, n_blocks; uint64_t total; };      // 32 bytes; the last 16 identify it

// ---- the single-frame decode's control blocks: small device buffers its kernels and the host talk through ----
// Every member stays at its byte offset (the assertions below): the layout is part of the kernels' machine code.

// The window kernel's verdict (k_decode_linked).  Inside IxCtl when an index ran; alone at the buffer's start when none did.
struct LinkedFallback { uint32_t gave_up, why, block; };       // 1: frame left to the generic kernel; (debug) which check stopped it, at which block

// the "gave up" bits of IxCtl::gave_up
constexpr uint32_t IX_UNUSABLE = 1u, IX_COPY_FAILED = 2u, IX_CHAIN_GATED = 4u;      // the index does not fit the frame; a copier or tracer failed; LZ4F_MI355X_CHAIN_GATE fired
constexpr uint32_t IXL_PUB = 8;                                // set-aside destinations a block publishes for the block behind (more: that one waits for all of it)

// -DSPX_PROF: k_spx_index's counters, at IxCtl's words 40..46 (cycles: max and sum / 256 of guess, walk, stitch; a workgroup's max) and 48..52
struct SpxProf { uint32_t _s[8], guess_max, walk_max, stitch_max, wg_max, guess_sum, walk_sum, stitch_sum, _s47, hop_cap, no_start, at_seg_start, ran_into, most_seqs; };

// The indexed decode's control block: 256 bytes, then (linked frames) the words ixctl_done() and its neighbours find.
struct IxCtl {
    uint32_t gave_up;                          // != 0: the generic decoders take the frame (the only_if word behind the indexed kernels)
    uint32_t _r1;
    uint32_t spx_stitched;                     // stretches walked by the stitching thread (LZ4F_MI355X_PROF prints it)
    uint32_t _r3;
    uint32_t m_direct, m_resolved, m_chain;    // (profile) matches direct after the parse, resolved, left to the chain
    uint32_t n_blocks;                         // k_check_index: the frame's block count
    // k_check_index writes the header's counts here, zero when it refuses it; k_selfindex_scan writes its totals to the same two words
    // (the host reads them to size the index it makes).  n_seqs is also the descriptor workspace's fill: the kernels' desc_cap.
    uint32_t n_entries, n_seqs;
    uint32_t chain_total;                      // k_dense_gate: the striped sample below, scaled up
    uint32_t m_reach_front, why_far, why_straddle, why_runlen, why_hops;      // (profile) chain matches into the block in front; not resolved because ...
    LinkedFallback window;                     // k_decode_linked behind the indexed kernels
    uint32_t _r19;
    uint32_t l_state3, l_state3_waited, l_setaside, l_front_done;            // (profile) k_copy_indexed, linked frames
    uint32_t dense;                            // != 0: a dense frame, decoded by the tracers (2: decided before k_resolve_direct, which was skipped)
    uint32_t dense_decided;                    // what the gate decided (kept for the host: the next call's hint)
    unsigned long long t_turns;                // (profile) k_trace_copy
    uint32_t t_pieces, t_from_out, t_deepest;
    uint32_t _r31;
    union {
        uint32_t chain[32];                    // matches left on the chain (striped; k_dense_gate sums them into chain_total)
        // -DSPX_PROF: k_spx_index's counters lie INSIDE the stripes.  The two never meet: a frame that k_spx_index walked has the buffer
        // cleared again before k_resolve_direct counts.
        SpxProf spx_prof;
    };
};
static_assert(sizeof(IxCtl) == 256, "control block layout");
#define LZ4F_AT(T, m, word) static_assert(offsetof(T, m) == 4 * (word), #T "::" #m " moved")
LZ4F_AT(IxCtl, gave_up, 0); LZ4F_AT(IxCtl, spx_stitched, 2); LZ4F_AT(IxCtl, m_direct, 4); LZ4F_AT(IxCtl, m_resolved, 5); LZ4F_AT(IxCtl, m_chain, 6);
LZ4F_AT(IxCtl, n_blocks, 7); LZ4F_AT(IxCtl, n_entries, 8); LZ4F_AT(IxCtl, n_seqs, 9); LZ4F_AT(IxCtl, chain_total, 10); LZ4F_AT(IxCtl, m_reach_front, 11);
LZ4F_AT(IxCtl, why_far, 12); LZ4F_AT(IxCtl, why_straddle, 13); LZ4F_AT(IxCtl, why_runlen, 14); LZ4F_AT(IxCtl, why_hops, 15); LZ4F_AT(IxCtl, window, 16);
LZ4F_AT(IxCtl, l_state3, 20); LZ4F_AT(IxCtl, l_state3_waited, 21); LZ4F_AT(IxCtl, l_setaside, 22); LZ4F_AT(IxCtl, l_front_done, 23);
LZ4F_AT(IxCtl, dense, 24); LZ4F_AT(IxCtl, dense_decided, 25); LZ4F_AT(IxCtl, t_turns, 26); LZ4F_AT(IxCtl, t_pieces, 28); LZ4F_AT(IxCtl, t_from_out, 29);
LZ4F_AT(IxCtl, t_deepest, 30); LZ4F_AT(IxCtl, chain, 32); LZ4F_AT(IxCtl, spx_prof.guess_max, 40); LZ4F_AT(IxCtl, spx_prof.stitch_sum, 46);
LZ4F_AT(IxCtl, spx_prof.hop_cap, 48); LZ4F_AT(IxCtl, spx_prof.most_seqs, 52);
LZ4F_AT(LinkedFallback, why, 1); LZ4F_AT(LinkedFallback, block, 2);
// Behind it, for the n_max groups of a linked frame: done[n_max] (k_copy_indexed's states), pcnt[n_max] (published ranges, or ~0: too
// many), then IXL_PUB ranges {from, to} per group.  The host clears done and pcnt for a linked frame's call.
LZ4F_FN uint32_t* ixctl_done(IxCtl* c) { return (uint32_t*)(c + 1); }
LZ4F_FN uint32_t* ixctl_pcnt(uint32_t* done, uint32_t n_max) { return done + n_max; }
LZ4F_FN uint32_t* ixctl_ranges(uint32_t* done, uint32_t n_max, uint32_t g) { return done + 2 * (size_t)n_max + (size_t)g * 2 * IXL_PUB; }
LZ4F_FN size_t ixctl_cleared(size_t n_max) { return sizeof(IxCtl) + n_max * 8; }
LZ4F_FN size_t ixctl_bytes(size_t n_max) { return sizeof(IxCtl) + n_max * (8 + 8 * IXL_PUB); }

// The finishing kernels' verdict words (k_xxh32_blocks*, k_finish_check -> k_finish_decode)
struct FinishVerdict {
    uint32_t ck_bad;                           // first block whose checksum is wrong (preset ~0)
    uint32_t first_bad;                        // first failed block (preset ~0)
    uint32_t moves;                            // != 0: something has to move
    uint32_t _r3;
    unsigned long long size_sum;               // sum of the decoded sizes
    uint32_t _r6[2];
};
static_assert(sizeof(FinishVerdict) == 32, "verdict layout");
LZ4F_AT(FinishVerdict, ck_bad, 0); LZ4F_AT(FinishVerdict, first_bad, 1); LZ4F_AT(FinishVerdict, moves, 2); LZ4F_AT(FinishVerdict, size_sum, 4);
constexpr size_t FINISH_ONES = offsetof(FinishVerdict, moves);      // the preset: this many bytes of 0xFF, zeros behind

// k_density_probe's verdict: exactly one of the two is 1 (each the only_if word of the decoder made for that kind of payload)
struct Density { uint32_t dense, not_dense, bytes_per_seq; };       // bytes_per_seq: payload bytes per sequence in the sample (0: no sequence seen)
LZ4F_AT(Density, dense, 0); LZ4F_AT(Density, not_dense, 1); LZ4F_AT(Density, bytes_per_seq, 2);
#undef LZ4F_AT

}  // namespace lz4f
