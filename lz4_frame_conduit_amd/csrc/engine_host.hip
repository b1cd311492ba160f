// engine_host.hip -- the engine's host-pointer layer: host buffers to the device and back around launch_compress / launch_decompress
// (engine.hip).  Staging copies, the link tokens, the slab and one-block calls of pipeline.hip and frame_host.cpp, and the trailer's
// block list made on the host.  No kernel is compiled here: HIP's runtime calls only.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>

#include "engine.hpp"

using namespace lz4f;

// The host-pointer calls are bounded by how fast bytes move between the caller's (pageable) buffers and the pinned staging
// buffers: one thread's memcpy is ~10 GB/s, a fifth of what the PCIe link takes.  Large copies are split over a few threads.
static void big_memcpy(void* dst, const void* src, size_t n)
{
    const size_t MIN_PER_THREAD = (size_t)8 << 20;
    unsigned hw = std::thread::hardware_concurrency();
    size_t t = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), n / MIN_PER_THREAD);
    if (t <= 1) { memcpy(dst, src, n); return; }
    const size_t per = ((n / t) + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (size_t i = 1; i < t; i++) {
        const size_t a = i * per;
        if (a >= n) break;
        const size_t len = std::min(per, n - a);
        th.emplace_back([=] { memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, len); });
    }
    memcpy(dst, src, std::min(per, n));
    for (auto& x : th) x.join();
}

// One upload and one download at a time per device.  Engines that share a device share its host link: two uploads side by
// side each take twice as long, and - symmetric as they are - the engines then also download side by side, so the link is never
// busy in both directions (measured: 32 GiB/s).  With a token per direction they fall out of step by themselves: one engine's
// upload runs beside the other's kernels and download.
namespace { std::mutex g_up_mu[16], g_down_mu[16]; }
static std::mutex& up_token(int device) { return g_up_mu[(unsigned)device % 16]; }
static std::mutex& down_token(int device) { return g_down_mu[(unsigned)device % 16]; }

// Is `p` page-locked memory the DMA engines can reach directly (hipHostMalloc / hipHostRegister: lz4f_mi355x_host_alloc,
// the conduits' batch buffers)?  Then no staging copy is needed.
bool lz4f::is_pinned_host(const void* p)
{
    hipPointerAttribute_t a; memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
// Host buffer <-> device through the pinned staging buffer, in pieces: the copy between the caller's pageable memory and the
// staging buffer (CPU threads) of one piece runs while the DMA of the piece before is in flight, instead of one after the other.
static const size_t XFER_PIECE = (size_t)32 << 20;
static hipError_t staged_h2d(void* d_dst, void* pinned, const void* src, size_t n, hipStream_t st)
{
    for (size_t a = 0; a < n; a += XFER_PIECE) {
        const size_t len = std::min(XFER_PIECE, n - a);
        big_memcpy((uint8_t*)pinned + a, (const uint8_t*)src + a, len);
        hipError_t e = hipMemcpyAsync((uint8_t*)d_dst + a, (uint8_t*)pinned + a, len, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
static hipError_t staged_d2h(void* dst, void* pinned, const void* d_src, size_t n, hipStream_t st)
{
    const size_t np = (n + XFER_PIECE - 1) / XFER_PIECE;
    std::vector<hipEvent_t> ev(np);
    hipError_t e = hipSuccess;
    size_t made = 0;
    for (size_t i = 0; i < np && e == hipSuccess; i++) {
        const size_t a = i * XFER_PIECE, len = std::min(XFER_PIECE, n - a);
        e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        if (e != hipSuccess) break;
        made++;
        e = hipMemcpyAsync((uint8_t*)pinned + a, (const uint8_t*)d_src + a, len, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(ev[i], st);
    }
    for (size_t i = 0; i < made; i++) {
        if (e == hipSuccess) e = hipEventSynchronize(ev[i]);
        if (e == hipSuccess) { const size_t a = i * XFER_PIECE, len = std::min(XFER_PIECE, n - a); big_memcpy((uint8_t*)dst + a, (uint8_t*)pinned + a, len); }
        (void)hipEventDestroy(ev[i]);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    return e;
}

size_t lz4f_mi355x_engine::slab_compress(const uint8_t* src, size_t n, const uint8_t* hist, size_t hist_len, uint32_t block_size, bool linked,
                                         bool block_checksum, bool src_pinned, size_t* size, int level)
{
    *size = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (!linked) hist_len = 0;
    if (hist_len > 65536) { hist += hist_len - 65536; hist_len = 65536; }
    const size_t total = hist_len + n;
    const size_t nblocks = (n + block_size - 1) / block_size;
    const size_t out_cap = n + nblocks * 8 + 64;
    if ((!src_pinned && h_in.ensure(total)) || h_small.ensure(65536 + 256) || d_in.ensure(total + 64) || d_out.ensure(out_cap) || res.ensure(sizeof(ResultRec)))
        return make_err(LZ4F_ERROR_allocation_failed);
    {
        std::lock_guard<std::mutex> up(up_token(device));
        if (hist_len) {
            if (src_pinned && hist + hist_len == src) HIP_TRY(hipMemcpyAsync(d_in.p, hist, hist_len, hipMemcpyHostToDevice, st));      // (the history sits in front of the input, in the same pinned buffer)
            else { memcpy(h_small.p, hist, hist_len); HIP_TRY(hipMemcpyAsync(d_in.p, h_small.p, hist_len, hipMemcpyHostToDevice, st)); }
        }
        if (src_pinned) HIP_TRY(hipMemcpyAsync((uint8_t*)d_in.p + hist_len, src, n, hipMemcpyHostToDevice, st));
        else HIP_TRY(staged_h2d((uint8_t*)d_in.p + hist_len, (uint8_t*)h_in.p + hist_len, src, n, st));
        if (n >= ((size_t)8 << 20)) HIP_TRY(hipStreamSynchronize(st));      // (bulk slabs: hold the token until the bytes are over)
    }
    const CompressJob j = make_compress_job((const uint8_t*)d_in.p, total, hist_len, block_size, linked, block_checksum, level);
    size_t r = launch_compress(j, (uint8_t*)d_out.p, out_cap, (lz4f_mi355x_result*)res.p, nullptr);
    if (is_err(r)) return r;
    ResultRec* hr = (ResultRec*)((uint8_t*)h_small.p + 65536 + 64);
    HIP_TRY(hipMemcpyAsync(hr, res.p, sizeof(ResultRec), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hr->status != ST_OK) { set_last_error("device compress status %u", hr->status); return make_err((int)hr->status); }
    *size = hr->size;
    return 0;
}

size_t lz4f_mi355x_engine::compress_block_pinned(const uint8_t* pin_src, size_t hist_len, size_t n, uint32_t block_size, bool linked, bool block_checksum,
                                                 uint8_t* pin_dst, size_t dst_cap, size_t* size, int level)
{
    // (Kernels reading the staging buffer through the link themselves - no copies at all - were tried first: 510 us per 64 KiB block
    // against 190 us with copies.  A kernel's scattered 16-byte reads over PCIe are not what a DMA engine's are.)
    *size = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (!linked) hist_len = 0;
    const size_t total = hist_len + n;
    const size_t out_cap = n + ((n + block_size - 1) / block_size) * 8 + 64;
    const size_t res_at = (out_cap + 63) & ~(size_t)63;                  // the result record rides behind the blocks: one copy back
    if (out_cap > dst_cap) return make_err(LZ4F_ERROR_dstMaxSize_tooSmall);
    if (d_in.ensure(total + 64) || d_out.ensure(res_at + sizeof(ResultRec) + 64)) return make_err(LZ4F_ERROR_allocation_failed);
    HIP_TRY(hipMemcpyAsync(d_in.p, pin_src, total, hipMemcpyHostToDevice, st));
    const CompressJob j = make_compress_job((const uint8_t*)d_in.p, total, hist_len, block_size, linked, block_checksum, level);
    lz4f_mi355x_result* d_res = (lz4f_mi355x_result*)((uint8_t*)d_out.p + res_at);
    size_t r = launch_compress(j, (uint8_t*)d_out.p, out_cap, d_res, nullptr);
    if (is_err(r)) return r;
    // (the blocks' size is not known on the host yet: everything up to the record comes back - at most a block and a few bytes)
    HIP_TRY(hipMemcpyAsync(pin_dst, d_out.p, res_at + sizeof(ResultRec), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const ResultRec* hr = (const ResultRec*)(pin_dst + res_at);
    if (hr->status != ST_OK) { set_last_error("device compress status %u", hr->status); return make_err((int)hr->status); }
    *size = hr->size;
    return 0;
}

size_t lz4f_mi355x_engine::slab_fetch(uint8_t* dst, size_t size, size_t d_off, bool dst_pinned)
{
    if (size == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (!dst_pinned && h_out.ensure(size + 64)) return make_err(LZ4F_ERROR_allocation_failed);
    std::lock_guard<std::mutex> down(down_token(device));
    if (dst_pinned) { HIP_TRY(hipMemcpyAsync(dst, (const uint8_t*)d_out.p + d_off, size, hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); return 0; }
    HIP_TRY(staged_d2h(dst, h_out.p, (const uint8_t*)d_out.p + d_off, size, st));
    return 0;
}

size_t lz4f_mi355x_engine::compress_blocks_host(const uint8_t* src, size_t n, const uint8_t* hist, size_t hist_len,
                                                uint32_t block_size, bool linked, bool block_checksum, uint8_t* dst, size_t dst_cap, size_t* written, int level)
{
    *written = 0;
    size_t size = 0;
    size_t r = slab_compress(src, n, hist, hist_len, block_size, linked, block_checksum, false, &size, level);
    if (is_err(r)) return r;
    if (size > dst_cap) return make_err(LZ4F_ERROR_dstMaxSize_tooSmall);
    r = slab_fetch(dst, size, 0, false);
    if (is_err(r)) return r;
    *written = size;
    return 0;
}

// One block of at most 256 KiB that comes back into the caller's buffer: the streaming API's call
static bool one_small_block(const uint8_t* fetch_to, size_t n_blocks, size_t max_block) { return fetch_to && n_blocks == 1 && max_block <= (256u << 10); }

// Where slab_decode puts things in its pinned staging buffer (h_in), and where the output starts in d_out.
//   one copy up (a small block out of pageable memory): [table | payload | history, right-aligned | output] is the staging buffer's AND
//     d_out's layout - table, payload and history go up in ONE copy: three copies of a few KiB each cost more in launches than in bytes;
//   otherwise: [payload (pageable input only) | table | history] staged, each with its own copy and device buffer; d_out is [history | output].
// The result record lands 8-byte aligned behind everything that is uploaded.
struct DecodeStaging { size_t table, payload, hist, out, rec, bytes; };      // offsets in h_in (out: in d_out); the bytes of h_in the call needs
static DecodeStaging decode_staging(bool one_up, bool src_pinned, size_t tbytes, size_t part_len, size_t hist_len)
{
    DecodeStaging s;
    if (one_up) {
        s.table = 0; s.payload = 64;
        s.out = ((((s.payload + part_len + 63 + 64) & ~(size_t)63) + hist_len + 63) & ~(size_t)63);
        s.hist = s.out - hist_len; s.rec = s.out + 64; s.bytes = s.out + 256;
    } else {
        s.payload = 0; s.table = src_pinned ? 0 : part_len; s.hist = s.table + tbytes;
        s.out = hist_len; s.rec = ((s.hist + hist_len) & ~(size_t)7) + 16; s.bytes = s.hist + hist_len + 128;
    }
    return s;
}

size_t lz4f_mi355x_engine::slab_decode(const uint8_t* frame_part, size_t part_len, const std::vector<lz4f_mi355x_block>& entries,
                                       const ParsedHeader& ph, const uint8_t* hist, size_t hist_len, bool src_pinned, size_t* got,
                                       uint8_t* fetch_to, size_t fetch_room, uint32_t* bad_block)
{   // fetch_to (one small block): the output comes back with the result record, before the ONE synchronisation of the call - a block's
    // worth is copied whatever the block decodes to, and what it did decode to goes to fetch_to
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const bool linked = ph.info.blockMode == LZ4F_blockLinked;
    if (!linked) hist_len = 0;
    const size_t nb = entries.size();
    // the device buffer always has room for every block at full size: blocks are decoded at provisional positions and
    // compacted when some are short (frames written with LZ4F_flush); only what is actually produced must fit the caller's buffer
    const size_t out_room = nb * ph.max_block;
    const size_t tbytes = nb * sizeof(BlockOut);
    const bool small = one_small_block(fetch_to, nb, ph.max_block), one_up = small && !src_pinned;
    const DecodeStaging at = decode_staging(one_up, src_pinned, tbytes, part_len, hist_len);
    if (h_in.ensure(at.bytes) || d_out.ensure(at.out + out_room + 64) || res.ensure(sizeof(ResultRec)) ||
        (!one_up && (d_in.ensure(part_len + 64) || table.ensure((nb + 1) * sizeof(BlockOut)))))
        return make_err(LZ4F_ERROR_allocation_failed);
    uint8_t* hp = (uint8_t*)h_in.p;
    memcpy(hp + at.table, entries.data(), tbytes);
    if (hist_len) memcpy(hp + at.hist, hist, hist_len);
    DecompressJob j; memset(&j, 0, sizeof(j));
    j.frame_cap = part_len; j.d_dst = (uint8_t*)d_out.p + at.out; j.dst_cap = out_room; j.hist0 = hist_len;
    j.block_size = (uint32_t)ph.max_block; j.linked = linked; j.block_checksum = ph.info.blockChecksumFlag != 0;
    j.n_blocks = (uint32_t)nb; j.max_blocks = (uint32_t)nb;
    if (one_up) {
        memcpy(hp + at.payload, frame_part, part_len);
        { std::lock_guard<std::mutex> up(up_token(device)); HIP_TRY(hipMemcpyAsync(d_out.p, hp, at.out, hipMemcpyHostToDevice, st)); }
        j.d_frame = (const uint8_t*)d_out.p + at.payload; j.table_direct = (lz4f_mi355x_block*)((uint8_t*)d_out.p + at.table);
    } else {
        std::lock_guard<std::mutex> up(up_token(device));
        if (src_pinned) HIP_TRY(hipMemcpyAsync(d_in.p, frame_part, part_len, hipMemcpyHostToDevice, st));
        else HIP_TRY(staged_h2d(d_in.p, hp + at.payload, frame_part, part_len, st));
        HIP_TRY(hipMemcpyAsync(table.p, hp + at.table, tbytes, hipMemcpyHostToDevice, st));
        if (hist_len) HIP_TRY(hipMemcpyAsync(d_out.p, hp + at.hist, hist_len, hipMemcpyHostToDevice, st));
        if (part_len >= ((size_t)8 << 20)) HIP_TRY(hipStreamSynchronize(st));
        j.d_frame = (const uint8_t*)d_in.p; j.table_in_place = true;
    }
    size_t r = launch_decompress(j, (lz4f_mi355x_result*)res.p);
    if (is_err(r)) return r;
    ResultRec* hr = (ResultRec*)(hp + at.rec);
    bool with_out = small;
    if (with_out && h_out.ensure(ph.max_block + 64)) { if (one_up) return make_err(LZ4F_ERROR_allocation_failed); with_out = false; }
    if (with_out) HIP_TRY(hipMemcpyAsync(h_out.p, j.d_dst, ph.max_block, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hr, res.p, sizeof(ResultRec), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hr->status != ST_OK) {
        if (bad_block) *bad_block = hr->first_bad_block;
        set_last_error("device decode status %u at block %u", hr->status, hr->first_bad_block); return make_err((int)hr->status);
    }
    *got = hr->size;
    if (fetch_to) {
        if (hr->size > fetch_room) return make_err(LZ4F_ERROR_dstMaxSize_tooSmall);
        if (with_out) memcpy(fetch_to, h_out.p, hr->size);
        else { const size_t r2 = slab_fetch(fetch_to, hr->size, at.out, false); if (is_err(r2)) return r2; }
    }
    return 0;
}

size_t lz4f_mi355x_engine::decompress_block_host(const uint8_t* payload, uint32_t csize, bool bck, const uint8_t* hist, size_t hist_len,
                                                 uint8_t* dst, uint32_t dst_cap, bool linked, uint32_t block_size, uint32_t* decoded)
{
    ParsedHeader ph; memset(&ph, 0, sizeof(ph));
    ph.max_block = block_size;
    ph.info.blockMode = linked ? LZ4F_blockLinked : LZ4F_blockIndependent;
    ph.info.blockChecksumFlag = bck ? LZ4F_blockChecksumEnabled : LZ4F_noBlockChecksum;
    std::vector<lz4f_mi355x_block> e(1);
    e[0].src_off = 0; e[0].dst_off = 0; e[0].word = csize; e[0].dst_size = dst_cap < block_size ? dst_cap : block_size;
    size_t got = 0;
    size_t r = slab_decode(payload, (size_t)csize + (bck ? 4 : 0), e, ph, hist, hist_len, false, &got, dst, dst_cap);
    if (is_err(r)) return r;
    *decoded = (uint32_t)got;
    return 0;
}

// ---- the trailer's block list made on the host (same bytes k_trailer_plan / k_trailer_copy write for a frame without a sequence index) ----
namespace lz4f {
bool BlockList::add_blocks(const uint8_t* b, size_t n, uint64_t frame_off, bool bck)
{
    size_t pos = 0;
    while (pos < n) {
        if (!frame_word_fits(n - pos)) return false;
        const uint32_t w = rd32le(b + pos);
        uint32_t csz; uint64_t step;                              // (a run of blocks without its header: any block size passes)
        if (is_endmark(w) || frame_block_word(w, 0x7FFFFFFFu, bck, n - pos - 4, csz, step)) return false;
        at.push_back(frame_off + pos);
        pos += 4 + (size_t)step;
    }
    return true;
}
size_t host_trailer_size(uint64_t F, uint64_t n_blocks)
{
    if (n_blocks == 0) return 0;
    if (n_blocks > 0x7FFFFFFFull) return make_err(LZ4F_ERROR_frameSize_wrong);
    const uint64_t list_at = (F + 8 + 15) & ~(uint64_t)15, n_list = (n_blocks + 1) & ~1ull;
    const uint64_t total = list_at + n_list * 8 + sizeof(TrailerFoot) - F;
    if (total - 8 >= 0xFFFFFFFFull) return make_err(LZ4F_ERROR_frameSize_wrong);        // (a skippable frame's size field is 32 bits)
    return (size_t)total;
}
void host_write_trailer(uint8_t* t, uint64_t F, const uint64_t* at, uint32_t n_blocks)
{
    const uint64_t list_at = (F + 8 + 15) & ~(uint64_t)15, n_list = ((uint64_t)n_blocks + 1) & ~1ull, ix_at = list_at + n_list * 8;
    const uint64_t total = ix_at + sizeof(TrailerFoot) - F;
    const uint32_t sz = (uint32_t)(total - 8);
    st32le(t, TR_MAGIC); st32le(t + 4, sz);
    memset(t + 8, 0, (size_t)(list_at - F - 8));
    for (uint64_t i = 0; i < n_list; i++) { const uint64_t v = i < n_blocks ? at[i] : 0; memcpy(t + (list_at - F) + i * 8, &v, 8); }
    const TrailerFoot f{0u, 0u, 0u, 0u, TR_FOOT, n_blocks, total};
    memcpy(t + (ix_at - F), &f, sizeof(f));
}
}  // namespace lz4f
