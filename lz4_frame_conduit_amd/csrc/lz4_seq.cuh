// lz4_seq.cuh -- the LZ4 block grammar's SEQUENCE HEADER, once: token, literal-length bytes, offset, match-length bytes.
//
// Every decode parser reads the header through these pieces; what a parser does with the lengths - which end-of-block rules it
// applies, where it takes the offset from, what it keeps wave-uniform - stays at its call site ("The sequence
// header", lists the differences).  wave_decode_block_lim (decode.cuh) is a different design, a byte at a time, and stands apart.
#pragma once
#include "common.cuh"

namespace lz4f {

// 8 payload bytes at `pos`, never touching memory at or beyond in + readable
__device__ __forceinline__ uint64_t pt_load8(const uint8_t* __restrict__ in, uint32_t pos, uint64_t readable)
{
    if ((uint64_t)pos + 8 <= readable) { typedef uint64_t u64u __attribute__((aligned(1))); return *(const u64u*)(in + pos); }
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; i++) if ((uint64_t)pos + i < readable) v |= (uint64_t)in[pos + i] << (8 * i);
    return v;
}

// 16 payload bytes at `pos` (same rule)
__device__ __forceinline__ void pt_load16(const uint8_t* __restrict__ in, uint32_t pos, uint64_t readable, uint64_t& lo, uint64_t& hi)
{
    if ((uint64_t)pos + 16 <= readable) { typedef uint64_t u64u __attribute__((aligned(1))); lo = *(const u64u*)(in + pos); hi = *(const u64u*)(in + pos + 8); return; }
    lo = pt_load8(in, pos, readable); hi = pt_load8(in, pos + 8, readable);
}

// ---- length bytes ----
// x: the candidate length bytes, first one lowest, with a byte that is not 0xFF among them (the callers shift the token - and the
// offset - out of an 8-byte read, so the top byte is 0).  k: how many 0xFF bytes lead; add: what the k + 1 bytes add to the 15 of
// the token's nibble.  k == 7 (literals, x = w >> 8) / k == 6 (match, x = w >> 16) means that the bytes run on beyond the read:
// `add` is then not the answer and len_ext_slow starts over.
struct LenExt { uint32_t k, add; };
__device__ __forceinline__ LenExt len_ext(uint64_t x)
{
    const uint32_t f = (uint32_t)__builtin_ctzll(~x), k = f >> 3;
    return LenExt{k, 255u * k + (uint32_t)((x >> (f & 56u)) & 0xFF)};
}

// The same byte by byte, from the first length byte (at `at`) on: returns `len` (what stands so far: 0, or the nibble's 15) grown by
// every byte; `after`: behind the last one.  `bad` is set when the payload ends first or the sum has passed `bound` (sum and
// `after` are then what they were where that was seen).  UNI: the walk is a wave's, every byte made wave-uniform; otherwise a lane's.
template <bool UNI>
__device__ __forceinline__ uint32_t len_ext_slow(const uint8_t* __restrict__ in, uint32_t csize, uint32_t at, uint32_t len, uint32_t bound, uint32_t& after, bool& bad)
{
    for (;;) {
        if (at >= csize || len > bound) { bad = true; break; }
        uint32_t b = in[at];
        if (UNI) b = uni(b);
        len += b; at++;
        if (b != 255) break;
    }
    after = at;
    return len;
}

// ---- the register window of the scalar-chain parsers ----
// Lane l holds the 16 payload bytes at wb + 8 * l (win.x .. win.w), so 8 bytes at any qq in [wb, wb + 504) are four v_readlane and
// a funnel shift.  The caller has made sure that qq is inside (each parser's `ensure` / `reload`).
// win_fetch_lo: only the bytes from qq to the end of its lane's first 8 - enough for the byte at qq.
template <class V4>
__device__ __forceinline__ uint64_t win_fetch_lo(const V4& win, uint32_t wb, uint32_t qq)
{
    const uint32_t rel = qq - wb, l = rel >> 3, sh8 = (rel & 7u) * 8u;
    const uint64_t lo = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(win.x, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(win.y, l) << 32);
    return lo >> sh8;
}
template <class V4>
__device__ __forceinline__ uint64_t win_fetch8(const V4& win, uint32_t wb, uint32_t qq)
{
    const uint32_t rel = qq - wb, l = rel >> 3, sh8 = (rel & 7u) * 8u;
    const uint64_t hi = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(win.z, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(win.w, l) << 32);
    return win_fetch_lo(win, wb, qq) | ((hi << 1) << (63u - sh8));
}

// ---- a lane's walk from sequence to sequence ----
// One dependent load per sequence: the 16 bytes at the match offset also hold the match-length bytes, the NEXT token and its
// literal-length bytes, so the cursor carries 8 of them over.  A sequence is read in two halves, and the caller loads w2, w2_hi =
// the 16 bytes at q = p + lit in between (with whatever it has to put around that load); a walk without a carried window calls
// the same halves on a fresh cursor.  Lengths beyond 2^24 are no block's: the byte-by-byte tails stop there.
struct SeqCur { uint32_t pos; uint64_t w; };               // the next token's position, 8 payload bytes from there on
__device__ __forceinline__ void seq_begin(const uint8_t* __restrict__ in, uint64_t readable, SeqCur& c) { c.w = pt_load8(in, c.pos, readable); }

// token, literal length, p: the first literal byte.  False: the length bytes are not a length (len_ext_slow).
template <bool UNI = false>
__device__ __forceinline__ bool seq_lit(const uint8_t* __restrict__ in, uint32_t csize, const SeqCur& c, uint32_t& token, uint32_t& lit, uint32_t& p)
{
    token = (uint32_t)c.w & 0xFF;
    lit = token >> 4; p = c.pos + 1;
    if (lit == 15) {
        const LenExt e = len_ext(c.w >> 8);
        if (e.k < 7) { lit += e.add; p += e.k + 1; }
        else { bool bad = false; lit = len_ext_slow<UNI>(in, csize, p, lit, 1u << 24, p, bad); return !bad; }
    }
    return true;
}

// mlen: the match length without its 4; the cursor goes to the next token (behind a byte-by-byte tail with a load, otherwise the
// token is 2..8 bytes into what is already here).  False: the length bytes are not a length; the cursor is then worth nothing.
template <bool UNI = false>
__device__ __forceinline__ bool seq_match(const uint8_t* __restrict__ in, uint32_t csize, uint64_t readable, SeqCur& c, uint32_t token, uint32_t q,
                                          uint64_t w2, uint64_t w2_hi, uint32_t& mlen)
{
    mlen = token & 15; c.pos = q + 2;
    if (mlen == 15) {
        const LenExt e = len_ext(w2 >> 16);
        if (e.k < 6) { mlen += e.add; c.pos += e.k + 1; }
        else {
            bool bad = false;
            mlen = len_ext_slow<UNI>(in, csize, c.pos, mlen, 1u << 24, c.pos, bad);
            if (bad) return false;
            seq_begin(in, readable, c);
            return true;
        }
    }
    const uint32_t sh = (c.pos - q) * 8u;
    c.w = sh >= 64 ? w2_hi : ((w2 >> sh) | (w2_hi << (64u - sh)));
    return true;
}

// ---- the lanes' path: 64 lanes look for the tokens of a 64-byte window (decode.cuh has the why) ----
// A lane reads the dword at its byte as if the byte were a token.  hdr: bytes in front of the literals (the token, and ONE literal-
// length byte where the nibble is 15 - a lane's own business, the byte is in its dword); lit: literals by that reading; ml: the
// match nibble; e1: the byte behind the token (hdr == 2 and e1 == 255: more length bytes follow, not a lane's business).
struct LaneTok { uint32_t hdr, lit, ml, e1; };
__device__ __forceinline__ LaneTok lane_token(uint32_t d)
{
    const uint32_t t = d & 0xFFu, litn = t >> 4, e1 = (d >> 8) & 0xFFu;
    return LaneTok{litn == 15u ? 2u : 1u, litn == 15u ? 15u + e1 : litn, t & 15u, e1};
}

// The serial part: one hop per token (v_readlane, s_bitset1, two moves, compare, branch).  nx: the lane the next token would be
// in if this lane's byte were one (64: exactly the window's end), 255 where the lane cannot tell.  A token is marked before its
// end is known; the last one is taken back if it does not end inside the window.  Returns the mask of tokens; s: the lane - the
// payload byte of the window - where the walk goes on.
__device__ __forceinline__ uint64_t hop_tokens(uint32_t nx, uint32_t& s)
{
    uint64_t mask = 0;
    uint32_t sp = 0, n;
    s = 0;
    do {
        n = (uint32_t)__builtin_amdgcn_readlane((int)nx, (int)s);
        asm("s_bitset1_b64 %0, %1" : "+s"(mask) : "s"(s));
        sp = s; s = n;
    } while (n < 64u);
    if (n > 64u) { mask &= ~(1ull << sp); s = sp; }
    return mask;
}

}  // namespace lz4f
