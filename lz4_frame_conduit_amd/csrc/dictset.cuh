// dictset.cuh -- a set of prepared dictionaries for the batch calls (lz4f_mi355x_dev_createDictSet): each frame of a batch names its
// own member by a slot, or by the dictID in its header.
//
// The set's device table (one allocation, uploaded once): DsMember[count] - per member what the kernels take of its CDict, the
// EncDict fields, and its ID - then the IDs sorted ascending and, beside each, the member that has it (the lookup is a binary search).
// The kernels take the table by value as a DsView.  A slot is a member index < count, DS_NONE (no dictionary), or DS_UNKNOWN (what a
// slot outside the set, or a header's ID that no member has, becomes: the frame fails, alone).  Every kernel holds a slot to
// `count` before it indexes the table, so a forged slot never reads outside it.
//   ds_find            an ID -> its member, or DS_UNKNOWN
//   ds_header_slot     a frame's span -> the slot its header names (no dictID field, a skippable frame, no valid header: DS_NONE)
//   ds_tail            a slot -> the member's bytes as the decoders take them (DictTail), wave-uniform
//   k_ds_resolve       a thread per frame: ds_header_slot into the caller's array (lz4f_mi355x_dev_resolveDictIDs)
#pragma once
#include "common.cuh"

namespace lz4f {

constexpr uint32_t DS_NONE = 0xFFFFFFFFu, DS_UNKNOWN = 0xFFFFFFFEu;      // LZ4F_MI355X_DICT_NONE, LZ4F_MI355X_DICT_UNKNOWN
constexpr uint32_t DS_MOST = 65536;                                      // members at most

struct DsMember {                           // per member (32 bytes): EncDict's fields, and the ID
    const uint8_t* end;                     // the member's bytes end here (len 0: a dictionary of no bytes)
    const uint4* solo_digest;
    const uint4* hc_digest;
    uint32_t len, id;
};
struct DsView {
    const DsMember* members = nullptr;
    const uint32_t* ids = nullptr;          // the IDs, ascending
    const uint32_t* order = nullptr;        // order[k]: the member whose ID is ids[k]
    uint32_t count = 0;
};

__device__ __forceinline__ uint32_t ds_find(const DsView& set, uint32_t id)
{
    uint32_t lo = 0, hi = set.count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (set.ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < set.count && set.ids[lo] == id ? set.order[lo] : DS_UNKNOWN;
}

// a caller's slot as the kernels keep it
__device__ __forceinline__ uint32_t ds_given_slot(uint32_t s, uint32_t count) { return s == DS_NONE || s < count ? s : DS_UNKNOWN; }

// The slot that the frame in f[0..cap) names: its header's dictID looked up in the set.  head_ok: the span begins with a header that
// stands (or a whole skippable frame) - where it does not, the frame fails with the header's own error and takes no dictionary
__device__ __forceinline__ uint32_t ds_header_slot(const uint8_t* __restrict__ f, uint64_t cap, const DsView& set, bool& head_ok)
{
    head_ok = false;
    if (cap < 7) return DS_NONE;
    if (is_skippable(rd32le(f))) { uint64_t c; head_ok = skippable_span(f, cap, c) == ST_OK; return DS_NONE; }
    FrameHead h;
    if (frame_head_parse(f, cap, h) != ST_OK) return DS_NONE;
    head_ok = true;
    return flg_dict(h.flg) ? ds_find(set, h.dict_id) : DS_NONE;
}

// a (wave-uniform) slot -> the member's bytes; DS_NONE, DS_UNKNOWN and whatever else is no member: none
__device__ __forceinline__ DictTail ds_tail(const DsView& set, uint32_t slot)
{
    DictTail t;
    if (slot < set.count) { t.end = (const uint8_t*)uni64((uint64_t)set.members[slot].end); t.len = uni(set.members[slot].len); }
    return t;
}

// a thread per frame: the slot its header names; a span that does not lie in the buffer is not read and gives DS_NONE
__global__ __launch_bounds__(256) void k_ds_resolve(const uint8_t* __restrict__ src, uint64_t src_bytes, const uint64_t* __restrict__ soff, uint32_t n_frames,
                                                    DsView set, uint32_t* __restrict__ slot)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    const uint64_t s0 = soff[i], s1 = soff[i + 1];
    uint32_t s = DS_NONE;
    if (s0 <= s1 && s1 <= src_bytes) { bool head_ok; s = ds_header_slot(src + s0, s1 - s0, set, head_ok); }
    slot[i] = s;
}

}  // namespace lz4f
