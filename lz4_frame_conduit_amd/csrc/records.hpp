// records.hpp -- the records and codes the kernels and the host-pointer layer share.  Plain C++: no device code, no HIP.
#pragma once
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

}  // namespace lz4f
