// encode_hc.cuh -- pass E1 for compression levels 3-12 (LZ4HC's levels): a hash-chain match finder with a lazy parse.
//
// One workgroup (16 waves) per 64 KiB chunk, which fills the chunk's ChunkInfo and record list exactly as pass E1 of encode.cuh and
// the deterministic finder of encode_solo.cuh do: passes S and E2, the raw fallback, checksums and the sequence index do not know the
// difference.  Matches reach up to 64 KiB back (into the block's earlier chunks, and across block starts when linked), end at the
// chunk's end, and keep Appendix A.2's end-of-block rules.
//
// LDS ("High-compression levels"):
//   chain  65536 + 1920 x u16   chain[q % HC_RING] = distance from q back to the previous position whose 4 bytes hash alike (0: none)
//   head    8 K x u16    16 KiB   per hash: the low 16 bits of the last position inserted
//   res  3 x 960 x u32   11.25 KiB per position of the last three batches: the best match found (length, offset, bytes it extends back)
// The 128 KiB input window stays in memory (L2): it does not fit beside the chain, and a candidate is checked with one 4-byte load.
//
// The window [chunk start - 64 KiB, chunk end) is walked in batches of HC_T = 960 positions.  In iteration i, all behind one barrier:
//   wave 0      inserts batch i into head/chain (in position order: the lanes of a group of 64 find the lane before them with the same
//               hash by ballots), then parses what the searchers have finished (batches <= i-2) into records;
//   waves 1-15  search batch i-1, a lane per position: the chain is walked for at most `attempts` candidates, and the longest match
//               (the nearest among equals) is kept.
// The builder writes the chain slots of batch i, which are the slots of positions HC_RING before it: the ring is two batches longer
// than 64 KiB, so those are out of reach of every position the searchers look at (full reach: 65535 bytes).  No wave ever reads what
// another writes in the same iteration, so the records are a function of the input, its history and the level alone: nothing depends
// on timing or on the pool.
//
// DICT (the batch encoder's prepared dictionary at these levels, encode_batch.cuh; it comes as one EncDict, encode.cuh, whose hc_digest
// is this finder's): the virtual history, the seam and the seam policy of encode_solo.cuh.  In front of a scope's first chunk (cs_abs == low_abs) lies the dictionary's tail: seam == back == min(64 KiB,
// dict_len), positions below `seam` address the dictionary.  Such a chunk loads head and chain[0 .. seam) from the dictionary's
// digest - their state once the dictionary's positions are in, made by this very build loop (DIGEST, k_hc_digest_dict) - and walks on
// from the batch that holds the seam.  A match is CUT at the seam: a candidate in the dictionary extends forwards to the dictionary's
// last byte at most and backwards within it, a candidate in the input does not extend backwards below the seam, and positions whose
// four bytes would straddle it are never inserted - so every load has one side.  Every other chunk has 64 KiB of input in front of it
// and never looks at the dictionary.  A dictionary of fewer than 4 bytes is ignored.
#pragma once
#include "encode.cuh"

namespace lz4f {

constexpr uint32_t HC_WAVES = 16, HC_T = 64 * (HC_WAVES - 1), HC_HASH_LOG = 13, HC_RING = 65536 + 2 * HC_T;
constexpr uint32_t HC_CAP = 258;          // longest match length a search records (8 bits: length - 3); the parse extends longer ones
constexpr uint32_t HC_BACK_CAP = 255;     // bytes a search records that its match extends backwards (8 bits)
constexpr uint32_t HC_LOOK = 2;           // positions the lazy parse looks ahead

// Level -> search attempts per position and lazy depth (1: one position ahead, 2: also two ahead).  Chosen by measured frame size
// against liblz4 1.9.3 at the same level (DESIGN.md section 4 has the sweep): 32 attempts with the one-ahead parse already meet level 3
// (real text x1.000-1.002, Zipf text x0.99); from level 6 the two-ahead parse, and attempts up to where more stop paying: on real text
// 256 -> 512 -> 2048 -> 8192 attempts gave x1.009 -> 1.007 -> 1.005 -> 1.0046 of liblz4's level-6 size at 1.0x, 1.3x, 3.3x, 11x the time.
// Levels above 12 are level 12.
struct HcLevel { uint32_t attempts, lazy; };
__host__ __device__ inline HcLevel hc_level(int level)
{
    const uint32_t att[10] = {32, 48, 64, 256, 384, 512, 1024, 2048, 4096, 8192};
    if (level < 3) level = 3;
    if (level > 12) level = 12;
    return HcLevel{att[level - 3], level >= 6 ? 2u : 1u};
}

struct alignas(16) HcShared {
    uint16_t chain[HC_RING];
    uint16_t head[1u << HC_HASH_LOG];
    uint32_t res[3][HC_T];
};
static_assert(sizeof(HcShared) <= 163840, "one workgroup per CU");
static_assert(HC_RING >= 65535 + 2 * HC_T, "the builder's slots are out of the searchers' reach");

__device__ __forceinline__ uint32_t hc_hash(uint32_t v) { return (v * 2654435761u) >> (32 - HC_HASH_LOG); }
__device__ __forceinline__ uint32_t hc_len(uint32_t r) { return r ? (r >> 24) + 3 : 0; }
__device__ __forceinline__ uint32_t hc_off(uint32_t r) { return r & 0xFFFFu; }
__device__ __forceinline__ uint32_t hc_back(uint32_t r) { return (r >> 16) & 0xFFu; }

// A dictionary's digest (the batch encoder's prepared dictionary, lz4f_mi355x_dev_createCDictHC): `head`, then chain[0 .. D) for the
// D = min(64 KiB, dict_len) bytes that count, as the build leaves them once positions 0 .. D-4 of the dictionary's tail are in, in
// position order.  A chunk with the dictionary alone in front of it counts its positions from the tail's first byte and D < HC_RING,
// so slot == position and the state is a function of the dictionary alone.  16-byte vectors, laid out in LDS as in memory.
constexpr uint32_t HC_DIGEST_HEAD_VEC = (uint32_t)(sizeof(uint16_t) << HC_HASH_LOG) / 16;
static_assert(HC_DIGEST_HEAD_VEC == 64 * HC_WAVES, "a thread per vector of head");
static_assert(offsetof(HcShared, chain) % 16 == 0 && offsetof(HcShared, head) % 16 == 0, "digest vectors");
__host__ __device__ inline uint32_t hc_digest_chain_vec(uint32_t D) { return (D * (uint32_t)sizeof(uint16_t) + 15u) / 16u; }
__host__ __device__ inline uint32_t hc_digest_bytes(uint32_t D) { return (HC_DIGEST_HEAD_VEC + hc_digest_chain_vec(D)) * 16u; }
static_assert(65536u * sizeof(uint16_t) + 15u < sizeof(HcShared::chain), "the last vector of a 64 KiB dictionary's chain lies in the ring");
// the workgroup's head and chain[0 .. D) <- the digest, every thread; four 16-byte loads in flight per thread.  The caller's barrier
// stands between these stores and the first halfword read
__device__ __forceinline__ void hc_digest_load(HcShared& sh, const uint4* __restrict__ digest, uint32_t D)
{
    const uint32_t tid = threadIdx.x, nvec = hc_digest_chain_vec(D);
    ((uint4*)sh.head)[tid] = digest[tid];
    const uint4* cv = digest + HC_DIGEST_HEAD_VEC;
    constexpr uint32_t T = 64 * HC_WAVES, F = 4;
    for (uint32_t q = 0; q < nvec; q += F * T) {
        uint4 vv[F];
#pragma unroll
        for (uint32_t u = 0; u < F; u++) { const uint32_t i = q + u * T + tid; vv[u] = cv[i < nvec ? i : 0u]; }
#pragma unroll
        for (uint32_t u = 0; u < F; u++) { const uint32_t i = q + u * T + tid; if (i < nvec) ((uint4*)sh.chain)[i] = vv[u]; }
    }
}

// One chunk, one workgroup of 64 * HC_WAVES threads: the search itself, for a chunk whose place is resolved (EncPlace, encode.cuh) - by
// k_find_matches_hc from the call's EncGeom, by the batch encoder from its chunk table (encode_batch.cuh).  `rec`: the chunk's record
// list (max_rec records of room; !rec_room: none, the chunk goes out as literals).  Every path ends behind a barrier or before the
// first use of `sh`, so a workgroup may call this for one chunk after another.
// DICT: the dc.len (<= 64 KiB) bytes that end at dc.end lie in front of a scope's first chunk, and dc.hc_digest holds head and chain as
// the dictionary leaves them (see above).  DIGEST (with DICT): clear, build the dictionary's positions, nothing else - how
// k_hc_digest_dict makes the digest, by the very code and in the very insertion order of the finders.
template <bool DICT = false, bool DIGEST = false>
__device__ __forceinline__ void hc_find_chunk(const uint8_t* __restrict__ src, const EncPlace& pl, ChunkInfo* __restrict__ ci,
                                              uint64_t* __restrict__ rec, const bool rec_room, const uint32_t max_rec,
                                              const uint32_t hc_attempts, const uint32_t lazy, HcShared& sh, const EncDict& dc)
{
    static_assert(DICT || !DIGEST, "a digest is a dictionary's");
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
    const uint64_t bstart = pl.bstart, bend_abs = pl.bend_abs, cs_abs = pl.cs_abs, ce_abs = pl.ce_abs, low_abs = pl.low_abs;
    uint32_t back = (uint32_t)((cs_abs - low_abs < 65536u) ? (cs_abs - low_abs) : 65536u);
    uint32_t seam = 0;                                               // DICT: positions below it are the dictionary's
    if constexpr (DICT) {
        if (dc.len >= 4 && cs_abs == low_abs) { seam = dc.len < 65536u ? dc.len : 65536u; back = seam; }
    }
    const uint8_t* base = src + (cs_abs - back);                     // position 0 of the window (DICT: positions from seam on)
    const uint8_t* dbase = DICT ? dc.end - seam : nullptr;           // DICT: position 0, for positions below seam
    const uint8_t* rd_end = src + pl.rd_end;                         // nothing is read at or beyond this
    auto at_pos = [&](uint32_t x) -> const uint8_t* { return DICT && x < seam ? dbase + x : base + x; };
    // 8 bytes of a match's source at position sp; in the dictionary: nothing at or beyond the seam (zeros instead)
    auto src8 = [&](uint32_t sp, bool in_dict) -> uint64_t {
        if (DICT && in_dict) return sp < seam ? ld64_guard(dbase + sp, dc.end) : 0ull;
        return ld64_guard(base + sp, rd_end);
    };
    const uint32_t cs = back, ce = back + (uint32_t)(ce_abs - cs_abs);
    const uint32_t bend = back + (uint32_t)(bend_abs - cs_abs);

    // a match may start at p iff cs <= p <= last_start, and may end at end_lim (as in encode_solo.cuh)
    const uint32_t blen = (uint32_t)(bend_abs - bstart), clen = ce - cs;
    bool searchable = blen >= MFLIMIT + 1 && clen >= MINMATCH && rec_room;
    uint32_t last_start = 0, end_lim = 0;
    if (searchable) {
        last_start = (ce - MINMATCH < bend - MFLIMIT) ? ce - MINMATCH : bend - MFLIMIT;
        end_lim = (ce < bend - LASTLIT) ? ce : bend - LASTLIT;
        searchable = last_start >= cs;
    }
    if constexpr (!DIGEST) {
        if (!searchable) {
            if (tid == 0) { ci->nrec = 0; ci->first_lit = 0; ci->tail_lit = ce - cs; ci->body_size = 0; }
            return;
        }
    }
    const uint32_t attempts = hc_attempts ? hc_attempts : 1u;

    // DICT, a chunk with the dictionary alone in front of it: head and chain[0 .. seam) come from the digest, which is their state
    // after positions 0 .. seam-4 went in (the last three would straddle the seam: never inserted); the walk starts at the batch
    // that holds the seam, and positions below ins_from are not inserted again
    uint32_t it0 = 0, ins_from = 0;
    bool cleared = false;
    if constexpr (DIGEST) {
        for (uint32_t k = tid; k < HC_RING / 2; k += 64 * HC_WAVES) ((uint32_t*)sh.chain)[k] = 0;
    } else if constexpr (DICT) {
        if (seam) { hc_digest_load(sh, dc.hc_digest, seam); it0 = seam / HC_T; ins_from = seam; cleared = true; }
    }
    if (!cleared)
        for (uint32_t k = tid; k < (1u << HC_HASH_LOG) / 2; k += 64 * HC_WAVES) ((uint32_t*)sh.head)[k] = 0;
    __syncthreads();

    // positions that can be a candidate (< some p <= last_start); DIGEST: the dictionary's, all but the last three
    const uint32_t insert_end = DIGEST ? (seam >= MINMATCH ? seam - (MINMATCH - 1) : 0u) : last_start + 1;
    const uint32_t nbatch = (insert_end + HC_T - 1) / HC_T;
    const uint32_t it_end = DIGEST ? nbatch : nbatch + 2;
    auto insertable = [&](uint32_t x) -> bool { return x < insert_end && (!DICT || x >= ins_from); };
    const uint64_t lt_mask = (1ull << lane) - 1;

    // parse state (wave 0; wave-uniform)
    uint32_t p = cs, anchor = cs, nrec = 0, first_lit = 0, body = 0;

    for (uint32_t it = it0; it < it_end; it++) {
        if (wave == 0) {
            // ---- build: insert batch `it` in position order ----
            if (it < nbatch) {
                constexpr uint32_t G = HC_T / 64;
                uint32_t vv[G];
#pragma unroll
                for (uint32_t k = 0; k < G; k++) { const uint32_t pos = it * HC_T + k * 64 + lane; vv[k] = insertable(pos) ? ld32(at_pos(pos)) : 0u; }
#pragma unroll 1
                for (uint32_t k = 0; k < G; k++) {
                    const uint32_t pos0 = it * HC_T + k * 64;
                    if (pos0 >= insert_end) break;
                    if (DICT && pos0 + 64 <= ins_from) continue;
                    const uint32_t pos = pos0 + lane;
                    const bool valid = insertable(pos);
                    const uint32_t h = hc_hash(vv[k]);
                    // the lane before me with my hash, and whether I am the last with it
                    uint64_t act = __ballot(valid);
                    uint32_t prev_lane = 64;
                    bool is_last = false;
                    while (act) {
                        const uint32_t L = (uint32_t)__builtin_ctzll(act);
                        const uint32_t hl = __builtin_amdgcn_readlane(h, L);
                        const bool mine = valid && h == hl;
                        const uint64_t m = __ballot(mine);
                        if (mine) {
                            const uint64_t below = m & lt_mask;
                            prev_lane = below ? 63u - (uint32_t)__builtin_clzll(below) : 64u;
                            is_last = (m >> lane) == 1ull;
                        }
                        act &= ~m;
                    }
                    const uint32_t hd = valid ? sh.head[h] : 0u;
                    if (valid) {
                        const uint32_t d = prev_lane < 64 ? lane - prev_lane : ((pos - hd) & 0xFFFFu);
                        sh.chain[pos % HC_RING] = (uint16_t)d;
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (valid && is_last) sh.head[h] = (uint16_t)pos;
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // ---- parse what is searched: positions < known_end have results ----
            const bool fin = it == nbatch + 1;
            const uint32_t known_end = fin ? 0xFFFFFFFFu : (it >= 1 ? (it - 1) * HC_T : 0u);
            const uint32_t res_end = last_start + 1;                     // results beyond: no match
            while (!DIGEST && p <= last_start && (fin || p + HC_LOOK < known_end) && nrec < max_rec) {
                const uint32_t w0 = p;
                const uint32_t x = w0 + lane;
                uint32_t v = 0;
                if (x < res_end && (fin || x < known_end)) v = sh.res[(x / HC_T) % 3][x % HC_T];
                // positions p in this window whose look-ahead is in the window and known
                uint32_t wend = w0 + 64 - HC_LOOK;
                if (!fin && known_end - HC_LOOK < wend) wend = known_end - HC_LOOK;
                while (p < wend && nrec < max_rec) {
                    const uint64_t bal = __ballot(v != 0 && x >= p && x < wend);
                    if (!bal) { p = wend; break; }
                    p = w0 + (uint32_t)__builtin_ctzll(bal);
                    uint32_t c = __builtin_amdgcn_readlane(v, p - w0);
                    bool moved = false;
                    while (hc_len(c) < HC_CAP) {
                        const uint32_t c1 = __builtin_amdgcn_readlane(v, p + 1 - w0);
                        if (hc_len(c1) > hc_len(c)) { p += 1; c = c1; moved = true; }
                        else if (lazy >= 2 && hc_len(__builtin_amdgcn_readlane(v, p + 2 - w0)) > hc_len(c) + 1) { p += 2; c = __builtin_amdgcn_readlane(v, p - w0); moved = true; }
                        else break;
                        if (p >= wend) break;
                    }
                    if (moved && p >= wend) break;                       // (its look-ahead is beyond the window: decided again after the reload)
                    uint32_t mlen = hc_len(c);
                    const uint32_t off = hc_off(c);
                    uint32_t bk = hc_back(c);
                    if (bk > p - anchor) bk = p - anchor;
                    uint32_t mp = p - bk;
                    if (mlen >= HC_CAP) {
                        // a long match: go on from its recorded end, 512 bytes per round (wave-wide, like encode_solo.cuh)
                        const bool cd = DICT && p - off < seam;          // a candidate in the dictionary: its match ends at the seam
                        while (true) {
                            const uint32_t b0 = p + mlen + lane * 8;
                            uint64_t y0 = 0;
                            if (b0 < end_lim) y0 = ld64_guard(base + b0, rd_end) ^ src8(b0 - off, cd);
                            uint32_t h0 = 0;
                            if (b0 < end_lim) { h0 = y0 ? (uint32_t)(__builtin_ctzll(y0) >> 3) : 8; const uint32_t r = end_lim - b0; if (h0 > r) h0 = r; }
                            if (DICT && cd && b0 < end_lim) { const uint32_t lim = b0 - off < seam ? seam - (b0 - off) : 0u; if (h0 > lim) h0 = lim; }
                            const uint64_t s0 = __ballot(h0 < 8);
                            if (s0) { const uint32_t f = (uint32_t)__builtin_ctzll(s0); mlen += f * 8 + __builtin_amdgcn_readlane(h0, f); break; }
                            mlen += WAVE * 8;
                        }
                    }
                    mlen += bk;
                    const uint32_t lit = mp - anchor;
                    if (lane == 0) rec[nrec] = pack_rec(lit, mlen, off);
                    if (nrec == 0) first_lit = lit;
                    body += seq_size(lit, mlen);
                    nrec++;
                    anchor = p = mp + mlen;
                }
            }
        } else if (!DIGEST && it >= 1 && it <= nbatch) {
            // ---- search batch it-1: a lane per position ----
            const uint32_t pos = (it - 1) * HC_T + (tid - 64);
            uint32_t r = 0;
            if (pos >= cs && pos <= last_start) {
                const uint32_t qmin = pos >= 65535u ? pos - 65535u : 0u;
                uint32_t maxlen = end_lim - pos;
                if (maxlen > HC_CAP) maxlen = HC_CAP;
                const uint32_t cur = ld32(base + pos);
                uint32_t best = 0, boff = 0, q = pos, tail = 0;
                for (uint32_t n = 0; n < attempts; n++) {
                    const uint32_t d = sh.chain[q % HC_RING];
                    if (d == 0 || d > q - qmin) break;
                    q -= d;
                    // DICT, a candidate in the dictionary: its match ends at the seam at the latest, so every load below lies in
                    // [dbase + q, dc.end) - and one that cannot beat `best` (or has no 4 bytes in front of the seam) is passed over
                    uint32_t cmax = maxlen;
                    const bool cd = DICT && q < seam;
                    if constexpr (DICT) {
                        if (cd) { if (seam - q < cmax) cmax = seam - q; if (cmax < MINMATCH || cmax <= best) continue; }
                    }
                    const uint8_t* qp = cd ? dbase + q : base + q;
                    const uint8_t* q_end = cd ? dc.end : rd_end;
                    if (ld32(qp) != cur) continue;
                    if (best >= MINMATCH && ld32(qp + best - 3) != tail) continue;
                    uint32_t len = MINMATCH;
                    while (len < cmax) {
                        const uint64_t y = ld64_guard(base + pos + len, rd_end) ^ ld64_guard(qp + len, q_end);
                        if (y) { len += (uint32_t)(__builtin_ctzll(y) >> 3); break; }
                        len += 8;
                    }
                    if (len > cmax) len = cmax;
                    if (len > best) {
                        best = len; boff = pos - q;
                        if (best >= maxlen) break;
                        tail = ld32(base + pos + best - 3);
                    }
                }
                if (best >= MINMATCH) {
                    // bytes the match extends backwards (bounded by the chunk's start and the window's; DICT: a source in the input
                    // stops at the seam, one in the dictionary at the dictionary's first byte)
                    const uint32_t qb = pos - boff;
                    const uint32_t qroom = DICT && qb >= seam ? qb - seam : qb;
                    uint32_t room = pos - cs; if (qroom < room) room = qroom; if (room > HC_BACK_CAP) room = HC_BACK_CAP;
                    uint32_t bk = 0;
                    while (bk < room && base[pos - 1 - bk] == *at_pos(qb - 1 - bk)) bk++;
                    r = ((best - 3) << 24) | (bk << 16) | boff;
                }
                sh.res[(pos / HC_T) % 3][pos % HC_T] = r;
            }
        }
        __syncthreads();
    }
    if constexpr (DIGEST) return;
    if (tid == 0) { ci->nrec = nrec; ci->first_lit = first_lit; ci->tail_lit = ce - anchor; ci->body_size = body; }
}

// The prepared dictionary's digest for levels 3-12: one workgroup runs the finder's own build over the dictionary's last dict_len
// (<= 64 KiB) bytes, which end at dict_end - an empty place at dict_end: cs_abs == low_abs, so seam == back == dict_len and no position
// is the input's - and stores head and chain[0 .. dict_len) to `digest` (hc_digest_bytes(dict_len), 16-byte aligned).  A dictionary of
// fewer than 4 bytes is ignored by the finder: its digest is the cleared tables.
__global__ __launch_bounds__(64 * HC_WAVES) void k_hc_digest_dict(const uint8_t* __restrict__ dict_end, uint32_t dict_len, uint4* __restrict__ digest)
{
    __shared__ HcShared sh;
    EncPlace pl;
    pl.bstart = 0; pl.bend_abs = 0; pl.cs_abs = 0; pl.ce_abs = 0; pl.low_abs = 0; pl.rd_end = 0;
    const uint32_t D = dict_len < 65536u ? dict_len : 65536u;
    const EncDict dc{DictTail{dict_end, D}};
    hc_find_chunk<true, true>(dict_end, pl, nullptr, nullptr, false, 0u, 0u, 0u, sh, dc);    // (ends behind a barrier)
    digest[threadIdx.x] = ((const uint4*)sh.head)[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < hc_digest_chain_vec(D); i += 64 * HC_WAVES) digest[HC_DIGEST_HEAD_VEC + i] = ((const uint4*)sh.chain)[i];
}

// grid: one workgroup of 64 * HC_WAVES threads per chunk; g.hc_attempts / g.hc_lazy from hc_level()
__global__ __launch_bounds__(64 * HC_WAVES) void k_find_matches_hc(const uint8_t* __restrict__ src, EncGeom g,
                                                                  ChunkInfo* __restrict__ info, uint64_t* __restrict__ recs)
{
    __shared__ HcShared sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = blockIdx.x;
    if (chunk >= g.n_chunks) return;
    ChunkInfo* ci = info + chunk;
    EncPlace pl;
    if (!enc_place(g, chunk, pl)) {         // chunk beyond a short last block
        if (tid == 0) { ci->nrec = 0; ci->first_lit = 0; ci->tail_lit = 0; ci->body_size = 0; }
        return;
    }
    // (a place of its own in the pool for this chunk's list: the engine sizes the pool for the worst case at these levels)
    const uint64_t rec_at = (uint64_t)chunk * g.max_rec_per_chunk;
    const bool rec_room = rec_at + g.max_rec_per_chunk <= g.rec_pool;
    uint64_t* rec = rec_pool_of(recs, g) + (rec_room ? rec_at : 0);
    if (tid == 0) rec_offs(recs)[chunk] = (uint32_t)(rec_room ? rec_at : 0);
    hc_find_chunk(src, pl, ci, rec, rec_room, g.max_rec_per_chunk, g.hc_attempts, g.hc_lazy, sh, EncDict{});
}

}  // namespace lz4f
