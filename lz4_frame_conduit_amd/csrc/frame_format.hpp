// frame_format.hpp -- the LZ4 frame grammar (lz4_Frame_format.md v1.6.1), once, for the host layer and the kernels alike: the
// constants, the header's parse and its writer, the rule for one hop over a size word, the frame's closing words, and the
// verdicts that depend on the grammar.  Plain C++ that also compiles under HIP; no kernel and no runtime call in here.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LZ4F_FN __host__ __device__ __forceinline__
#else
#define LZ4F_FN inline
#endif

namespace lz4f {

// status codes: the values of LZ4F_errorCodes that a frame can earn
enum : uint32_t {
    ST_OK = 0, ST_GENERIC = 1, ST_MAXBLOCK = 2, ST_VERSION = 6, ST_BLOCKCK = 7, ST_RESERVED = 8, ST_SRCLARGE = 10, ST_DSTSMALL = 11,
    ST_INCOMPLETE = 12, ST_FRAMETYPE = 13, ST_FRAMESIZE = 14, ST_SRCPTR = 15, ST_DECOMP = 16, ST_HEADERCK = 17, ST_CONTENTCK = 18
};

constexpr uint32_t FRAME_MAGIC = 0x184D2204u, SKIP_MAGIC = 0x184D2A50u, SKIP_MASK = 0xFFFFFFF0u;
constexpr uint32_t FLAG_SKIPPABLE = 0x100;          // a result record's flags: FLG in the low byte, this bit for a skippable frame
LZ4F_FN bool is_skippable(uint32_t magic) { return (magic & SKIP_MASK) == SKIP_MAGIC; }

// FLG: version(2) independent blockChecksum contentSize contentChecksum reserved dictID.  BD: reserved blockSizeID(3) reserved(4)
LZ4F_FN uint32_t flg_version(uint32_t flg) { return (flg >> 6) & 3; }
LZ4F_FN uint32_t flg_indep(uint32_t flg) { return (flg >> 5) & 1; }
LZ4F_FN uint32_t flg_bck(uint32_t flg) { return (flg >> 4) & 1; }
LZ4F_FN uint32_t flg_csize(uint32_t flg) { return (flg >> 3) & 1; }
LZ4F_FN uint32_t flg_cck(uint32_t flg) { return (flg >> 2) & 1; }
LZ4F_FN uint32_t flg_reserved(uint32_t flg) { return (flg >> 1) & 1; }
LZ4F_FN uint32_t flg_dict(uint32_t flg) { return flg & 1; }
LZ4F_FN uint32_t make_flg(bool indep, bool bck, bool csize, bool cck, bool dict)
{
    return (1u << 6) | ((uint32_t)indep << 5) | ((uint32_t)bck << 4) | ((uint32_t)csize << 3) | ((uint32_t)cck << 2) | (uint32_t)dict;
}
LZ4F_FN uint32_t bd_bsid(uint32_t bd) { return (bd >> 4) & 7; }
LZ4F_FN uint32_t bsid_block_size(uint32_t bsid) { return 1u << (8 + 2 * bsid); }      // bsid 4..7

// a size word: bit 31 = stored, the rest the payload's bytes; zero is the EndMark
LZ4F_FN bool is_endmark(uint32_t w) { return w == 0; }
LZ4F_FN uint32_t word_size(uint32_t w) { return w & 0x7FFFFFFFu; }
LZ4F_FN bool word_stored(uint32_t w) { return (w >> 31) != 0; }

LZ4F_FN uint32_t rd32le(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
LZ4F_FN uint64_t rd64le(const uint8_t* p) { return (uint64_t)rd32le(p) | ((uint64_t)rd32le(p + 4) << 32); }
LZ4F_FN void st32le(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// ---- XXH32: the constants, and the whole function for the descriptor's fewer than 16 bytes ----
constexpr uint32_t XP1 = 2654435761u, XP2 = 2246822519u, XP3 = 3266489917u, XP4 = 668265263u, XP5 = 374761393u;
LZ4F_FN uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
LZ4F_FN uint32_t xxh32_small(const uint8_t* p, uint32_t len)   // len < 16, seed 0
{
    uint32_t h = XP5 + len, i = 0;
    for (; i + 4 <= len; i += 4) h = rotl32(h + rd32le(p + i) * XP3, 17) * XP4;
    for (; i < len; i++) h = rotl32(h + p[i] * XP5, 11) * XP1;
    h ^= h >> 15; h *= XP2; h ^= h >> 13; h *= XP3; h ^= h >> 16;
    return h;
}
// the header checksum: the second byte of XXH32 over the descriptor, FLG up to the byte in front of it
LZ4F_FN uint8_t frame_head_checksum(const uint8_t* p, uint32_t hsize) { return (uint8_t)(xxh32_small(p + 4, hsize - 5) >> 8); }

// ---- the header ----
struct FrameHead { uint32_t hsize, bs, bsid, flg, bck, dict_id; uint64_t content; };
LZ4F_FN uint32_t frame_head_size(uint32_t flg) { return 7 + (flg_csize(flg) ? 8 : 0) + (flg_dict(flg) ? 4 : 0); }

// The header of an LZ4 frame in p[0..n) -> ST_OK and the fields, or the error, in LZ4F_decodeHeader's order.  A skippable frame is
// the caller's branch (is_skippable, skippable_span): here it is frameType_unknown.  ST_INCOMPLETE with n >= 7 means n <
// frame_head_size(p[4]), and that magic, reserved bit and version have passed.
LZ4F_FN uint32_t frame_head_parse(const uint8_t* p, uint64_t n, FrameHead& h)
{
    if (n < 7) return ST_INCOMPLETE;
    if (rd32le(p) != FRAME_MAGIC) return ST_FRAMETYPE;
    h.flg = p[4];
    if (flg_reserved(h.flg)) return ST_RESERVED;
    if (flg_version(h.flg) != 1) return ST_VERSION;
    h.hsize = frame_head_size(h.flg);
    if (n < h.hsize) return ST_INCOMPLETE;
    const uint32_t bd = p[5];
    h.bsid = bd_bsid(bd);
    if ((bd >> 7) & 1) return ST_RESERVED;
    if (h.bsid < 4) return ST_MAXBLOCK;
    if (bd & 15) return ST_RESERVED;
    if (frame_head_checksum(p, h.hsize) != p[h.hsize - 1]) return ST_HEADERCK;
    h.bs = bsid_block_size(h.bsid);
    h.bck = flg_bck(h.flg);
    h.content = flg_csize(h.flg) ? rd64le(p + 6) : 0;
    h.dict_id = flg_dict(h.flg) ? rd32le(p + h.hsize - 5) : 0;
    return ST_OK;
}

// The header for `flg` (make_flg) and a block size ID, checksum included -> its bytes (at most 19).  The content size and the
// dictID are written where FLG says they are there.
LZ4F_FN uint32_t frame_head_write(uint8_t* dst, uint32_t flg, uint32_t bsid, uint64_t content, uint32_t dict_id)
{
    st32le(dst, FRAME_MAGIC);
    dst[4] = (uint8_t)flg; dst[5] = (uint8_t)((bsid & 7u) << 4);
    uint32_t n = 6;
    if (flg_csize(flg)) { st32le(dst + n, (uint32_t)content); st32le(dst + n + 4, (uint32_t)(content >> 32)); n += 8; }
    if (flg_dict(flg)) { st32le(dst + n, dict_id); n += 4; }
    dst[n] = frame_head_checksum(dst, n + 1);
    return n + 1;
}

// a skippable frame in p[0..n), n >= 7: magic, u32 size, payload -> ST_OK and the bytes it takes
LZ4F_FN uint32_t skippable_span(const uint8_t* p, uint64_t n, uint64_t& consumed)
{
    if (n < 8) return ST_INCOMPLETE;
    consumed = 8 + (uint64_t)rd32le(p + 4);
    return n < consumed ? ST_INCOMPLETE : (uint32_t)ST_OK;
}

// ---- the frame directory of a packed stream (lz4f_mi355x_dev_packFrames with LZ4F_MI355X_PACK_DIRECTORY) ----
// One skippable frame in front of the frames: u32 magic, u32 payloadBytes = 16 + 4 * n_frames, then the payload: u32 tag, u32
// n_frames, u64 framesBytes (the sum of the lengths), u32 L[n_frames].  Little-endian, at any alignment.  (0xE is the trailer's.)
constexpr uint32_t PACKDIR_MAGIC = SKIP_MAGIC | 0xDu, PACKDIR_TAG = 0x44505A4Cu;       // "LZPD"
constexpr uint32_t PACKDIR_HEAD = 24, PACKDIR_MOST = (0xFFFFFFFFu - 16u) / 4u;          // the fixed part; the most frames a payload's u32 size can say
LZ4F_FN uint64_t pack_dir_size(uint32_t n_frames) { return PACKDIR_HEAD + 4ull * n_frames; }
LZ4F_FN uint64_t pack_dir_len_at(uint32_t i) { return PACKDIR_HEAD + 4ull * i; }       // where L[i] stands
LZ4F_FN void pack_dir_head_write(uint8_t* p, uint32_t n_frames, uint64_t frames_bytes)
{
    st32le(p, PACKDIR_MAGIC); st32le(p + 4, 16u + 4u * n_frames);
    st32le(p + 8, PACKDIR_TAG); st32le(p + 12, n_frames);
    st32le(p + 16, (uint32_t)frames_bytes); st32le(p + 20, (uint32_t)(frames_bytes >> 32));
}
// the fixed part in p[0..n) -> ST_OK, the frames and the sum of their lengths as the directory states them; or ST_INCOMPLETE for fewer
// than 24 bytes, ST_FRAMETYPE for another magic or tag, ST_FRAMESIZE where the payload's size is not that of n_frames lengths
LZ4F_FN uint32_t pack_dir_head_parse(const uint8_t* p, uint64_t n, uint32_t& n_frames, uint64_t& frames_bytes)
{
    if (n < PACKDIR_HEAD) return ST_INCOMPLETE;
    if (rd32le(p) != PACKDIR_MAGIC || rd32le(p + 8) != PACKDIR_TAG) return ST_FRAMETYPE;
    n_frames = rd32le(p + 12);
    frames_bytes = rd64le(p + 16);
    if (n_frames > PACKDIR_MOST || rd32le(p + 4) != 16u + 4u * n_frames) return ST_FRAMESIZE;
    return ST_OK;
}

// ---- the blocks ----
// One hop: the size word `w` of a frame of block size `bs`, `bytes_left` of the frame behind the word -> ST_OK, the payload's size
// and how far behind the word the next word is (payload and block checksum); or why the walk ends here.  The EndMark is ST_OK
// with nothing behind it (is_endmark tells it from an empty stored block).  The next word needs its four bytes: frame_word_fits.
LZ4F_FN uint32_t frame_block_word(uint32_t w, uint32_t bs, uint32_t bck, uint64_t bytes_left, uint32_t& csz, uint64_t& advance)
{
    csz = word_size(w);
    advance = is_endmark(w) ? 0 : (uint64_t)csz + 4 * bck;
    if (csz > bs) return ST_MAXBLOCK;
    if (bytes_left < advance) return ST_INCOMPLETE;
    return ST_OK;
}
LZ4F_FN bool frame_word_fits(uint64_t bytes_left) { return bytes_left >= 4; }

// behind the EndMark: the content checksum's word, when FLG asks for one -> ST_OK and the bytes it takes
LZ4F_FN uint32_t frame_end(uint32_t flg, uint64_t bytes_left, uint32_t& tail)
{
    tail = flg_cck(flg) ? 4 : 0;
    return bytes_left < tail ? (uint32_t)ST_INCOMPLETE : (uint32_t)ST_OK;
}

// ---- verdicts ----
// A block that failed at `at` in a window of `win` bytes.  kind: -2 it decodes, but not into its room; -3 it does not decode
// even with a whole block of room; anything else: it did not decode into the room it had.  Less room than a whole block is "the
// output does not fit", as liblz4 and the oracle call it (oracle/orc_lz4frame.c).
LZ4F_FN uint32_t block_fail_status(int32_t kind, uint64_t at, uint64_t win, uint32_t bs)
{
    const bool short_room = at <= win && win - at < bs && kind != -3;
    return (kind == -2 || short_room) ? ST_DSTSMALL : ST_GENERIC;
}
// the decoded size against the header's content size, when FLG says there is one
LZ4F_FN uint32_t frame_size_status(uint32_t flg, uint64_t declared, uint64_t decoded)
{
    return (flg_csize(flg) && declared != decoded) ? ST_FRAMESIZE : ST_OK;
}

}  // namespace lz4f
