// encode_batch.cuh -- many independent inputs, one frame each, in one call (lz4f_mi355x_dev_compressFrames), no host read in between.
//
// The single-frame call makes its plan on the host from one input's length; here every frame's geometry is made on the device,
// and every kernel takes all frames at once (the scan and the slice check are batch_common.cuh's, shared with the batch decoder):
//   k_bc_head      a thread per frame: the span and the window checked against the buffers; blocks, chunks and records counted
//   k_bc_place     one workgroup: exclusive scans of the three counts -> each frame's slice of the block table, of the chunk table
//                  (and of the ChunkInfo array beside it) and of the record pool.  The host sizes them from the call's arguments alone:
//                  every valid block size has 64 KiB chunks, so spans that do not overlap never need more than
//                  n_frames + srcBytes / 64 KiB + 1 chunks, no more blocks than that, and srcBytes / 4 records + one per chunk (the
//                  worst case of every chunk: a list never comes up short, ENC_POOL_SHORT never appears).  Only spans that overlap can
//                  exceed them: entries go out in frame order, and the first frame that does not get its own and the frames behind it
//                  fail, ERROR_srcSize_tooLarge, without touching the frames in front.  ctl[0], ctl[1]: the chunk and block entries
//                  in use - the grids below are sized by the bound and stride over these
//   k_bc_table     a wave per frame writes its block and chunk entries: a chunk's entry is its resolved place (EncPlace) - its bytes,
//                  its block, how far back a match may reach (the block's start, or 64 KiB into the SAME input when linked), where
//                  reads end (the span's end) - and where its record list lives
//   k_bc_find_*    the deterministic match finders over the chunk table: solo_find_chunk (encode_solo.cuh, a wave per chunk, levels
//                  <= 2) or hc_find_chunk (encode_hc.cuh, a workgroup per chunk, levels 3-12) - the very functions the single call's
//                  kernels run, so a frame's records are what they would be alone
//                  Two kernel templates of one signature, k_bc_find_solo<DICT, CDICT, D> and k_bc_find_hc<DICT, D>; the call's
//                  dictionary reaches them as one EncDict (encode.cuh), D, from which bc_frame_dict gives each chunk its frame's.  k_bc_find_solo<true, false>: the call's shared dictionary in front of every
//                  low_abs; <true, true>: a prepared dictionary, whose digested table a scope's first chunk copies;
//                  k_bc_find_hc<true>: levels 3-12 with a prepared dictionary that carries the hash-chain digest
//   k_bc_layout    a wave per block: layout_block_chunks (pass S's per-block step: carries, raw fallback) -> the size word
//   k_bc_frames    a wave per frame: the blocks placed behind the header, the window judged, then header (made here: content size and
//                  HC byte are the frame's own), size words, EndMark, every chunk's place in the destination, the result record
//   k_bc_emit      a wave per chunk: emit_chunk (pass E2)
//   k_bc_blockck   a wave per block: the block checksums (only when asked for)
//   k_bc_content   a wave per frame: the content checksums, side by side (only when asked for)
// A set of dictionaries (lz4f_mi355x_dev_compressFrames_usingDictSet, dictset.cuh): frame i has the member its slot names.  Three
// launches come in a set form - k_bc_head_set (the slot held to the set, kept in BcFrame::slot), the finders with D = DsView,
// k_bc_find_solo<true, true, DsView> / k_bc_find_hc<true, DsView> (bc_frame_dict: the chunk's frame's EncDict from the set's table),
// and k_bc_frames<W, true> (the member's ID in the header) - the others are shared.
// Nothing is written outside a frame's window on its behalf, and nothing at all unless the whole frame fits it.
// Limits: no sequence index, no in-band trailer, no block table comes out, and the finders are the deterministic ones only.  A big
// input of many blocks gets a wave for its layout and one for its content checksum: send it through lz4f_mi355x_dev_compressFrame,
// which puts the shared finder on it.
#pragma once
#include "common.cuh"
#include "encode.cuh"
#include "encode_solo.cuh"
#include "encode_hc.cuh"
#include "batch_common.cuh"
#include "dictset.cuh"

namespace lz4f {

constexpr uint32_t BC_NONE = BF_NONE;
constexpr uint32_t BC_CHUNK = 65536;        // pick_chunk_size() of every valid block size
constexpr uint32_t BC_CHUNK_RECS = BC_CHUNK / 4 + 1;

struct BcFrame {                            // per frame (device workspace, 72 bytes)
    uint64_t src, len;                      // the input's span in d_src
    uint64_t dst, win;                      // the frame's window in d_dst
    uint64_t rec_at;                        // its first record in the pool (until k_bc_place: how many it needs)
    uint64_t fsize;                         // the frame's bytes (k_bc_frames)
    uint32_t status, n_blocks, n_chunks;
    uint32_t blk_at, chk_at, slot;          // first block / chunk entry, BC_NONE: none; slot: the set calls' slot (bc_head_body), else 0
};
static_assert(sizeof(BcFrame) == 72, "BcFrame: 72 bytes");
struct BcBlk {                              // block table entry (32 bytes)
    uint64_t src, out;                      // the block in d_src; its payload's place in d_dst (k_bc_frames)
    uint32_t blen, word, frame, chk_at;     // input bytes, size word (k_bc_layout), frame, first chunk entry
};
struct BcChunk {                            // chunk table entry (64 bytes): EncPlace + the record list
    uint64_t cs_abs, bstart, low_abs, rd_end, rec_at;
    uint32_t clen, blen, frame, max_rec;
    uint32_t pad[2];
};
// what one batch's frames have in common (the call's preferences, resolved on the host)
struct BcPrefs {
    uint32_t block_size, bsid, linked, block_checksum, content_checksum, content_size, dict_id;
    uint32_t hc_attempts, hc_lazy;          // levels 3-12 (0: level <= 2)
};

// an entry of this call: its frame is alive and its slice holds the entry
__device__ __forceinline__ bool bc_chunk_live(const BcFrame* __restrict__ frames, uint32_t n_frames, uint32_t fi, uint32_t w)
{
    return fi < n_frames && uni(frames[fi].status) == 0 && slice_holds(uni(frames[fi].chk_at), uni(frames[fi].n_chunks), w);
}
__device__ __forceinline__ bool bc_blk_live(const BcFrame* __restrict__ frames, uint32_t n_frames, uint32_t fi, uint32_t w)
{
    return fi < n_frames && uni(frames[fi].status) == 0 && slice_holds(uni(frames[fi].blk_at), uni(frames[fi].n_blocks), w);
}

// SET (k_bc_head_set, the set calls): behind the offset checks the frame's slot, slot[i], is held to the set and kept in r.slot - a
// member, DS_NONE, or DS_UNKNOWN for anything else, which fails the frame (ST_GENERIC: k_bc_frames marks its record)
template <bool SET>
__device__ __forceinline__ void bc_head_body(uint64_t src_bytes, const uint64_t* __restrict__ soff, uint64_t dst_bytes,
                                             const uint64_t* __restrict__ doff, uint32_t n_frames, const BcPrefs& pf, BcFrame* __restrict__ frames,
                                             const uint32_t* __restrict__ slot, uint32_t n_members)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    BcFrame r;
    r.src = 0; r.len = 0; r.dst = 0; r.win = 0; r.rec_at = 0; r.fsize = 0;
    r.status = 0; r.n_blocks = 0; r.n_chunks = 0; r.blk_at = BC_NONE; r.chk_at = BC_NONE; r.slot = SET ? DS_NONE : 0;
    const uint64_t s0 = soff[i], s1 = soff[i + 1], d0 = doff[i], d1 = doff[i + 1];
    if (s0 > s1 || s1 > src_bytes) r.status = ST_SRCPTR;                 // nothing is read or written
    else if (d0 > d1 || d1 > dst_bytes) r.status = ST_DSTSMALL;
    else if (SET && (r.slot = ds_given_slot(slot[i], n_members)) == DS_UNKNOWN) r.status = ST_GENERIC;
    else {
        r.src = s0; r.len = s1 - s0; r.dst = d0; r.win = d1 - d0;
        const uint64_t nb = (r.len + pf.block_size - 1) / pf.block_size, full = r.len / BC_CHUNK, rem = r.len % BC_CHUNK;
        if (nb > 0x7FFFFFFFull / (pf.block_size / BC_CHUNK)) r.status = ST_SRCLARGE;      // more chunks than a 32-bit count holds (as the single call's plan)
        else {
            r.n_blocks = (uint32_t)nb; r.n_chunks = (uint32_t)(full + (rem ? 1 : 0));
            r.rec_at = full * BC_CHUNK_RECS + (rem ? rem / 4 + 1 : 0);   // the worst case of every chunk: a record per 4 bytes, + 1
        }
    }
    frames[i] = r;
}
__global__ __launch_bounds__(256) void k_bc_head(uint64_t src_bytes, const uint64_t* __restrict__ soff, uint64_t dst_bytes,
                                                 const uint64_t* __restrict__ doff, uint32_t n_frames, BcPrefs pf, BcFrame* __restrict__ frames)
{
    bc_head_body<false>(src_bytes, soff, dst_bytes, doff, n_frames, pf, frames, nullptr, 0u);
}
__global__ __launch_bounds__(256) void k_bc_head_set(uint64_t src_bytes, const uint64_t* __restrict__ soff, uint64_t dst_bytes,
                                                     const uint64_t* __restrict__ doff, uint32_t n_frames, BcPrefs pf, BcFrame* __restrict__ frames,
                                                     const uint32_t* __restrict__ slot, uint32_t n_members)
{
    bc_head_body<true>(src_bytes, soff, dst_bytes, doff, n_frames, pf, frames, slot, n_members);
}

// one workgroup: exclusive scans of the frames' blocks, chunks and records; a frame whose slices would end beyond a table or the pool
// (only spans that overlap can do that) fails.  Entries are handed out in frame order and a refused frame still counts in the scans
// (not counting it would make every frame's place depend on the verdicts in front of it: a serial pass), so every frame with input
// behind the first one that does not fit is refused too; the frames in front of it are untouched.
// ctl[0]: chunk entries in use, ctl[1]: block entries
__global__ __launch_bounds__(1024) void k_bc_place(BcFrame* __restrict__ frames, uint32_t n_frames, uint64_t blk_cap, uint64_t chk_cap,
                                                   uint64_t rec_cap, uint32_t* __restrict__ ctl)
{
    __shared__ WgScan<3> s;
    wg_scan_begin(s);
    for (uint32_t base = 0; base < n_frames; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const bool in = i < n_frames && frames[i].status == 0;
        const uint64_t c[3] = {in ? frames[i].n_blocks : 0u, in ? frames[i].n_chunks : 0u, in ? frames[i].rec_at : 0ull};
        uint64_t at[3];
        wg_scan_tile(c, at, s);
        if (in && c[1]) {
            if (at[0] + c[0] <= blk_cap && at[1] + c[1] <= chk_cap && at[2] + c[2] <= rec_cap) {
                frames[i].blk_at = (uint32_t)at[0]; frames[i].chk_at = (uint32_t)at[1]; frames[i].rec_at = at[2];
            } else frames[i].status = ST_SRCLARGE;
        }
    }
    if (threadIdx.x == 0) { ctl[0] = (uint32_t)(s.carry[1] < chk_cap ? s.carry[1] : chk_cap); ctl[1] = (uint32_t)(s.carry[0] < blk_cap ? s.carry[0] : blk_cap); }
}

// a wave per frame: its block entries and its chunk entries
template <int W>
__global__ __launch_bounds__(64 * W) void k_bc_table(const BcFrame* __restrict__ frames, uint32_t n_frames, BcPrefs pf, BcBlk* __restrict__ blocks,
                                                     BcChunk* __restrict__ chunks)
{
    const uint32_t i = uni(blockIdx.x * W + (threadIdx.x >> 6));
    if (i >= n_frames) return;
    const uint32_t lane = lane_id();
    const uint32_t status = uni(frames[i].status), nb = uni(frames[i].n_blocks), nc = uni(frames[i].n_chunks);
    const uint32_t blk_at = uni(frames[i].blk_at), chk_at = uni(frames[i].chk_at);
    if (status != 0 || chk_at == BC_NONE) return;
    const uint64_t s0 = uni64(frames[i].src), len = uni64(frames[i].len), rec0 = uni64(frames[i].rec_at);
    const uint32_t bs = pf.block_size, cpb = bs / BC_CHUNK;
    for (uint32_t b = lane; b < nb; b += WAVE) {
        const uint64_t at = (uint64_t)b * bs;
        BcBlk e;
        e.src = s0 + at; e.out = 0; e.blen = (uint32_t)(len - at < bs ? len - at : bs); e.word = 0; e.frame = i; e.chk_at = chk_at + b * cpb;
        blocks[blk_at + b] = e;
    }
    for (uint32_t c = lane; c < nc; c += WAVE) {
        const uint64_t cs = (uint64_t)c * BC_CHUNK, bat = cs / bs * bs;
        BcChunk e;
        e.cs_abs = s0 + cs; e.bstart = s0 + bat; e.low_abs = pf.linked ? s0 : s0 + bat; e.rd_end = s0 + len;
        e.rec_at = rec0 + (uint64_t)c * BC_CHUNK_RECS;                    // (every chunk in front of this one is a full one)
        e.clen = (uint32_t)(len - cs < BC_CHUNK ? len - cs : BC_CHUNK); e.blen = (uint32_t)(len - bat < bs ? len - bat : bs);
        e.frame = i; e.max_rec = e.clen / 4 + 1; e.pad[0] = 0; e.pad[1] = 0;
        chunks[chk_at + c] = e;
    }
}

__device__ __forceinline__ EncPlace bc_place_of(const BcChunk& e)
{
    EncPlace pl;
    pl.bstart = uni64(e.bstart); pl.bend_abs = pl.bstart + uni(e.blen);
    pl.cs_abs = uni64(e.cs_abs); pl.ce_abs = pl.cs_abs + uni(e.clen);
    pl.low_abs = uni64(e.low_abs); pl.rd_end = uni64(e.rd_end);
    return pl;
}

// The dictionary of a chunk's frame, as the finders below take it (wave-uniform).  Their last argument is the source, D: the call's
// one EncDict, which is every frame's - or, for a set of dictionaries (lz4f_mi355x_dev_compressFrames_usingDictSet), the set's table,
// from which the wave (the workgroup) loads its chunk's frame's member by the frame's slot (BcFrame::slot, held to the set by
// k_bc_head_set) and runs the prepared-dictionary finder with it: solo_find_chunk<true, true> / hc_find_chunk<true>.  Those ask the
// dictionary for a scope's first chunk only (cs_abs == low_abs) and then load ITS digest over the whole table, or clear the table when
// the frame has no member or one of fewer than 4 bytes (dc.len < 4: seam 0, the finder runs as without a dictionary) - so a workgroup
// that strides from a chunk of one member to a chunk of another carries nothing over, as the one-dictionary forms carry nothing from
// chunk to chunk.  (At levels 3-12 the host lets only hash-chain CDicts in as non-empty members: dc.hc_digest is there when seam is.)
__device__ __forceinline__ const EncDict& bc_frame_dict(const EncDict& dc, const BcFrame* __restrict__, uint32_t) { return dc; }
__device__ __forceinline__ EncDict bc_frame_dict(const DsView& set, const BcFrame* __restrict__ frames, uint32_t fi)
{
    EncDict dc;
    const uint32_t s = uni(frames[fi].slot);
    if (s < set.count) {
        const DsMember* m = set.members + s;
        dc.end = (const uint8_t*)uni64((uint64_t)m->end); dc.len = uni(m->len);
        dc.solo_digest = (const uint4*)uni64((uint64_t)m->solo_digest); dc.hc_digest = (const uint4*)uni64((uint64_t)m->hc_digest);
    }
    return dc;
}

// The deterministic finder of levels <= 2 over the chunk table: a wave per chunk (a one-wave workgroup, as the single call launches it:
// 11.25 KiB of LDS per wave bound the occupancy).  Its instantiations (the two finder kernels share one signature, so that the
// host picks one and launches it: `pf` is k_bc_find_hc's, `dcs` is for DICT):
//   <false, false>  no dictionary (lz4f_mi355x_dev_compressFrames)
//   <true, false>   the batch's shared dictionary (lz4f_mi355x_dev_compressFrames_usingDict; it was k_bc_find_solo_dict): the dc.len
//                   (<= 64 KiB) bytes that end at dc.end lie in front of every chunk's low_abs (solo_find_chunk<true>).  The dictionary
//                   is the call's, not a chunk's: the chunk table and the workspace are what they are without it
//   <true, true>    a prepared dictionary (lz4f_mi355x_dev_compressFrames_usingCDict; it was k_bc_find_solo_cdict): dc.solo_digest is
//                   the seeded table of a chunk that has the dictionary alone in front of it (k_solo_digest_dict), and such a chunk -
//                   cs_abs == low_abs: every frame's first chunk, and every independent block's - copies it into LDS, 11.25 KiB, where
//                   <true, false> reads up to 64 KiB of dictionary and inserts some 17 000 seeds.  (Chunks are 64 KiB, so a chunk
//                   behind the first of its scope has 64 KiB of input in front and no dictionary: it seeds as ever.  The finder asks
//                   cs_abs == low_abs itself and does not lean on that.)  Table and tags are one array here, in the digest's layout;
//                   the same 11 520 bytes of LDS.  (The other two keep their two arrays: the one-array form costs the plain kernel
//                   two VGPRs and an SGPR)
//   <true, true, DsView>  a set of prepared dictionaries (it was k_bc_find_solo_set): <true, true> with each chunk's frame's member
template <bool DICT, bool CDICT, typename D = EncDict>
__global__ __launch_bounds__(64) void k_bc_find_solo(const uint8_t* __restrict__ src, const BcFrame* __restrict__ frames, uint32_t n_frames,
                                                     const BcChunk* __restrict__ chunks, const uint32_t* __restrict__ ctl,
                                                     ChunkInfo* __restrict__ info, uint64_t* __restrict__ pool, BcPrefs pf, D dcs)
{
    static_assert(DICT || !CDICT, "a digest is a dictionary's");
    uint16_t* table; uint8_t* tags;
    if constexpr (CDICT) {
        __shared__ uint4 s_dig[SOLO_DIGEST_VEC];
        table = solo_digest_table(s_dig); tags = solo_digest_tags(s_dig);
    } else {
        __shared__ uint16_t s_table[SOLO_HASH_SIZE];
        __shared__ uint8_t s_tag[SOLO_HASH_SIZE];
        table = s_table; tags = s_tag;
    }
    const uint32_t total = uni(ctl[0]);
    for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
        const BcChunk e = chunks[w];
        const uint32_t fi = uni(e.frame);
        if (!bc_chunk_live(frames, n_frames, fi, w)) continue;
        const EncPlace pl = bc_place_of(e);
        decltype(auto) dc = bc_frame_dict(dcs, frames, fi);
        solo_find_chunk<DICT, CDICT>(src, pl, info + w, pool + uni64(e.rec_at), true, uni(e.max_rec), table, tags, dc);
    }
}

// Levels 3-12: a workgroup per chunk.  DICT (it was k_bc_find_hc_cdict): a prepared dictionary that carries the hash-chain digest
// (lz4f_mi355x_dev_createCDictHC).  A chunk with the dictionary alone in front of it - cs_abs == low_abs: every frame's first chunk, and
// every independent block's - loads dc.hc_digest (head and chain[0 .. D), k_hc_digest_dict) into the workgroup's LDS where the plain
// kernel clears head, and walks on from the batch that holds the seam.  All of it is loaded again for every such chunk, so nothing
// depends on the chunks this workgroup had before; every other chunk has 64 KiB of input in front of it and runs as without DICT.  The
// same HcShared: the digest needs no LDS of its own.  <true, DsView> (it was k_bc_find_hc_set): each chunk's frame's member
template <bool DICT, typename D = EncDict>
__global__ __launch_bounds__(64 * HC_WAVES) void k_bc_find_hc(const uint8_t* __restrict__ src, const BcFrame* __restrict__ frames, uint32_t n_frames,
                                                              const BcChunk* __restrict__ chunks, const uint32_t* __restrict__ ctl,
                                                              ChunkInfo* __restrict__ info, uint64_t* __restrict__ pool, BcPrefs pf, D dcs)
{
    __shared__ HcShared sh;
    const uint32_t total = uni(ctl[0]);
    for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
        const BcChunk e = chunks[w];
        const uint32_t fi = uni(e.frame);
        if (!bc_chunk_live(frames, n_frames, fi, w)) continue;
        const EncPlace pl = bc_place_of(e);
        decltype(auto) dc = bc_frame_dict(dcs, frames, fi);
        hc_find_chunk<DICT>(src, pl, info + w, pool + uni64(e.rec_at), true, uni(e.max_rec), pf.hc_attempts, pf.hc_lazy, sh, dc);
        __syncthreads();                                                  // (the chunk that had nothing to search left without a barrier)
    }
}
// what the two have in common, for the host: the finder of a dictionary source D
template <typename D>
using BcFinder = void (*)(const uint8_t*, const BcFrame*, uint32_t, const BcChunk*, const uint32_t*, ChunkInfo*, uint64_t*, BcPrefs, D);

// a wave per block: pass S's per-block step
template <int W>
__global__ __launch_bounds__(64 * W) void k_bc_layout(const BcFrame* __restrict__ frames, uint32_t n_frames, BcBlk* __restrict__ blocks,
                                                      const uint32_t* __restrict__ ctl, ChunkInfo* __restrict__ info)
{
    const uint32_t total = uni(ctl[1]);
    for (uint32_t w = uni(blockIdx.x * W + (threadIdx.x >> 6)); w < total; w += gridDim.x * W) {
        const uint32_t fi = uni(blocks[w].frame);
        if (!bc_blk_live(frames, n_frames, fi, w)) continue;
        const uint32_t blen = uni(blocks[w].blen);
        const uint32_t word = layout_block_chunks(info + uni(blocks[w].chk_at), (blen + BC_CHUNK - 1) / BC_CHUNK, blen);
        if (lane_id() == 0) blocks[w].word = word;
    }
}

// a wave per frame: where its blocks go, whether the window holds the frame, and everything of the frame that is not a block's payload.
// SET (k_bc_frames<W, true>): the header's dictID is the frame's member's ID (DS_NONE: the call's, pf.dict_id), and a frame whose slot was
// no member gets the unknown-slot record
// (One kernel template, the set an empty struct in the plain form: a shared body behind two kernels changed the plain form's code.)
template <bool SET> struct BcFramesSet {};
template <> struct BcFramesSet<true> : DsView {};
template <int W, bool SET>
__global__ __launch_bounds__(64 * W) void k_bc_frames(uint8_t* dst, BcFrame* __restrict__ frames, uint32_t n_frames, BcPrefs pf, BcBlk* __restrict__ blocks,
                                                      ChunkInfo* __restrict__ info, ResultRec* __restrict__ results, BcFramesSet<SET> set)
{
    const uint32_t i = uni(blockIdx.x * W + (threadIdx.x >> 6));
    if (i >= n_frames) return;
    const uint32_t lane = lane_id();
    const uint32_t status = uni(frames[i].status), nb = uni(frames[i].n_blocks), nc = uni(frames[i].n_chunks);
    const uint32_t blk_at = uni(frames[i].blk_at), chk_at = uni(frames[i].chk_at);
    const uint64_t len = uni64(frames[i].len), d0 = uni64(frames[i].dst), win = uni64(frames[i].win);
    uint32_t set_id = 0;                                                  // SET: the header's dictID
    if constexpr (SET) {
        set_id = pf.dict_id;
        const uint32_t s = uni(frames[i].slot);
        if (s < set.count) set_id = uni(set.members[s].id);
        else if (s != DS_NONE) {
            if (lane == 0) results[i] = ResultRec{0ull, 0ull, (uint32_t)ST_GENERIC, 0u, 0xFFFFFFFFu, (LZ4F_MI355X_PATH_BATCH | LZ4F_MI355X_PATH_DICT_UNKNOWN) << 12};
            return;
        }
    }
    const uint32_t dict_id = SET ? set_id : pf.dict_id;
    auto flg_with = [&](bool csize) { return make_flg(!pf.linked, pf.block_checksum, csize, pf.content_checksum, (SET ? set_id : pf.dict_id) != 0); };
    if (status != 0) {                                                    // (no frame: the call's FLG)
        if (lane == 0) results[i] = ResultRec{0ull, 0ull, status, 0u, 0xFFFFFFFFu, flg_with(pf.content_size) | (LZ4F_MI355X_PATH_BATCH << 12)};
        return;
    }
    // (an empty input's header declares no content size: a contentSize of 0 is "not given", to the single call too)
    const uint32_t flg = flg_with(pf.content_size && len != 0), flags = flg | (LZ4F_MI355X_PATH_BATCH << 12);
    const uint32_t hs = frame_head_size(flg);
    // the blocks, one behind the other behind the header
    uint64_t at = d0 + hs;
    for (uint32_t b0 = 0; b0 < nb; b0 += WAVE) {
        const uint32_t b = b0 + lane;
        const uint32_t bytes = b < nb ? 4u + (blocks[blk_at + b].word & 0x7FFFFFFFu) + 4u * pf.block_checksum : 0u;
        uint32_t sum;
        const uint32_t before = wave_excl_scan(bytes, sum);
        if (b < nb) blocks[blk_at + b].out = at + before + 4;            // the payload follows the size word
        at += sum;
    }
    const uint64_t fsize = at - d0 + 4 + (pf.content_checksum ? 4 : 0);
    const bool fits = fsize <= win;
    __threadfence();                                                      // (the lanes read each other's entries below)
    if (fits) {
        if (lane == 0) {                                                  // the header: made in registers, then stored
            uint8_t h[20];
            const uint32_t n = frame_head_write(h, flg, pf.bsid, len, dict_id);
            for (uint32_t q = 0; q < n; q++) dst[d0 + q] = h[q];
        }
        for (uint32_t b = lane; b < nb; b += WAVE) st32le(dst + blocks[blk_at + b].out - 4, blocks[blk_at + b].word);
        if (lane < 4) dst[at + lane] = 0;                                 // EndMark
    }
    // every chunk's place (layout_chunk)
    const uint32_t cpb = pf.block_size / BC_CHUNK;
    for (uint32_t c = lane; c < nc; c += WAVE) {
        ChunkInfo* ci = info + chk_at + c;
        if (!fits) { ci->flags |= 4u; continue; }
        const uint32_t b = c / cpb, cib = c % cpb;
        const BcBlk e = blocks[blk_at + b];
        ci->out_off = (e.word >> 31) ? e.out + (uint64_t)cib * BC_CHUNK : e.out + ci->out_off;
    }
    if (lane == 0) {
        frames[i].fsize = fsize;
        if (!fits) frames[i].status = ST_DSTSMALL;
        results[i] = ResultRec{fits ? fsize : 0ull, len, fits ? (uint32_t)ST_OK : (uint32_t)ST_DSTSMALL, nb, 0xFFFFFFFFu, flags};
    }
}

// a wave per chunk: pass E2
template <int W>
__global__ __launch_bounds__(64 * W) void k_bc_emit(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const BcFrame* __restrict__ frames,
                                                    uint32_t n_frames, const BcChunk* __restrict__ chunks, const uint32_t* __restrict__ ctl,
                                                    const ChunkInfo* __restrict__ info, const uint64_t* __restrict__ pool)
{
    __shared__ uint4 s_gt[W][2][64];
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t total = uni(ctl[0]);
    for (uint32_t w = uni(blockIdx.x * W + wv); w < total; w += gridDim.x * W) {
        const BcChunk e = chunks[w];
        if (!bc_chunk_live(frames, n_frames, uni(e.frame), w)) continue;
        const EncPlace pl = bc_place_of(e);
        const ChunkInfo ci = info[w];
        emit_chunk<false>(src, pl, ci, pool + uni64(e.rec_at), dst, nullptr, 0u, 0u, 0ull, 0u, s_gt[wv][0], s_gt[wv][1], 0u, 1u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();     // (the tables are the next chunk's)
    }
}

// a wave per block: XXH32 of the payload behind it.  LANE4: big blocks, the four-lane chain (lane4_xxh32)
template <int W, bool LANE4>
__global__ __launch_bounds__(64 * W) void k_bc_blockck(uint8_t* dst, const BcFrame* __restrict__ frames, uint32_t n_frames, const BcBlk* __restrict__ blocks,
                                                       const uint32_t* __restrict__ ctl)
{
    __shared__ __attribute__((aligned(16))) uint32_t park[W][LANE4 ? XXH_PARK / 4 : 1];
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t total = uni(ctl[1]);
    for (uint32_t w = uni(blockIdx.x * W + wv); w < total; w += gridDim.x * W) {
        const uint32_t fi = uni(blocks[w].frame);
        if (!bc_blk_live(frames, n_frames, fi, w)) continue;
        const uint64_t off = uni64(blocks[w].out);
        const uint32_t n = uni(blocks[w].word) & 0x7FFFFFFFu;
        uint32_t h;
        if constexpr (LANE4) h = lane4_xxh32(dst + off, n, park[wv]); else h = wave_xxh32(dst + off, n);
        if (lane_id() == 0) st32le(dst + off + n, h);
    }
}

// a wave per frame: XXH32 of the input, behind the EndMark
template <int W>
__global__ __launch_bounds__(64 * W) void k_bc_content(const uint8_t* __restrict__ src, uint8_t* dst, const BcFrame* __restrict__ frames, uint32_t n_frames)
{
    __shared__ __attribute__((aligned(16))) uint32_t park[W][XXH_PARK / 4];
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t i = uni(blockIdx.x * W + wv);
    if (i >= n_frames) return;
    if (uni(frames[i].status) != 0) return;
    const uint32_t h = lane4_xxh32(src + uni64(frames[i].src), uni64(frames[i].len), park[wv]);
    if (lane_id() == 0) st32le(dst + uni64(frames[i].dst) + uni64(frames[i].fsize) - 4, h);
}

}  // namespace lz4f
