// engine.hip -- kernels (via the .cuh headers), the engine's lifecycle, the two launch drivers and the device-pointer C ABI
// (the host-pointer layer around the drivers: engine_host.hip).
// Target: gfx950 only (MI355X).  No CPU fallback: without a usable device every entry fails loudly.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "engine.hpp"
#include "frame_dev.cuh"
#include "decode_batch.cuh"
#include "encode_batch.cuh"
#include "measure_batch.cuh"
#include "pack_batch.cuh"
#include "split_batch.cuh"
#include "train_dict.cuh"

using namespace lz4f;

static_assert(sizeof(ChunkInfo) == 32, "chunk info layout");
static_assert(sizeof(BatchFrame) == 80 && sizeof(BatchBlk) == 40, "batch workspace layout");
static_assert(sizeof(BatchCore) == 64 && sizeof(MeasBlk) == 24, "batch measure workspace layout");
static_assert(sizeof(BcFrame) == 72 && sizeof(BcBlk) == 32 && sizeof(BcChunk) == 64, "batch encode workspace layout");

namespace lz4f {

static thread_local char t_err[512] = "";
static thread_local int t_device = -1;

void set_last_error(const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(t_err, sizeof(t_err), fmt, ap); va_end(ap);
}
const char* last_error() { return t_err; }

// grow-only: room for n bytes and an eighth more, what was there is freed first (its contents are not kept)
static int grow(void** p, size_t* cap, size_t n, bool pinned)
{
    if (n <= *cap) return 0;
    const size_t want = n + n / 8 + 4096;
    if (*p) (void)(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr; *cap = 0;
    const hipError_t e = pinned ? hipHostMalloc(p, want, hipHostMallocDefault) : hipMalloc(p, want);
    if (e != hipSuccess) { set_last_error("%s(%zu) failed: %s", pinned ? "hipHostMalloc" : "hipMalloc", want, hipGetErrorString(e)); *p = nullptr; return 1; }
    *cap = want;
    return 0;
}
int DevBuf::ensure(size_t n) { return grow(&p, &cap, n, false); }
int PinBuf::ensure(size_t n) { return grow(&p, &cap, n, true); }
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
void PinBuf::release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }

int selected_device()
{
    if (t_device < 0) {
        const char* s = getenv("LZ4F_MI355X_DEVICE");
        t_device = s ? atoi(s) : 0;
    }
    return t_device;
}

uint32_t pick_chunk_size(uint32_t block_size)
{
    const uint32_t c = 64u << 10;    // pass E1's tile (E1_TILE): what one workgroup searches at a time, and the unit of passes S and E2
    return block_size < c ? block_size : c;
}

}  // namespace lz4f
void lz4f_mi355x_engine::Switches::read()
{
    auto on = [](const char* n) { return getenv(n) != nullptr; };
    auto num = [](const char* n, int lo, int hi, int dflt) { const char* v = getenv(n); if (!v) return dflt; const int k = atoi(v); return k >= lo && k <= hi ? k : dflt; };      // an integer in [lo, hi], else the default
    no_index = on("LZ4F_MI355X_NO_INDEX");
    no_selfindex = on("LZ4F_MI355X_NO_SELFINDEX");
    no_resolve = on("LZ4F_MI355X_NO_RESOLVE");
    no_trace = on("LZ4F_MI355X_NO_TRACE");
    no_doubling = on("LZ4F_MI355X_NO_DOUBLING");
    trace_always = on("LZ4F_MI355X_TRACE_ALWAYS");
    no_groups = on("LZ4F_MI355X_NO_GROUPS");
    no_window = on("LZ4F_MI355X_NO_WINDOW");
    serial_walk = on("LZ4F_MI355X_SERIAL_WALK");
    no_trailer = on("LZ4F_MI355X_NO_TRAILER");
    no_density_probe = on("LZ4F_MI355X_NO_DENSITY_PROBE");
    no_spx = on("LZ4F_MI355X_NO_SPX");
    no_overlap = on("LZ4F_MI355X_NO_OVERLAP");
    no_content_check = on("LZ4F_MI355X_NO_CONTENT_CHECK");
    split_serial = on("LZ4F_MI355X_SPLIT_SERIAL");
    prof = on("LZ4F_MI355X_PROF");
    e1_sync = on("LZ4F_MI355X_E1_SYNC");
    no_selffeed = on("LZ4F_MI355X_NO_SELFFEED");
    dense_mode = (unsigned)num("LZ4F_MI355X_DENSE_MODE", 0, 2, 0);
    group_kib = (unsigned)num("LZ4F_MI355X_GROUP_KIB", 64, 4096, 0);
    if (group_kib & (group_kib - 1)) group_kib = 0;                  // (a power of two)
    feed_round = (unsigned)num("LZ4F_MI355X_FEED_ROUND", 17, 4096, 0);
    chain_gate = num("LZ4F_MI355X_CHAIN_GATE", 1, (1 << 20) - 1, 0);
    decode_mode = 0; if (const char* v = getenv("LZ4F_MI355X_DECODE")) decode_mode = v[0];
    e1_run = (unsigned)num("LZ4F_MI355X_E1_RUN", 1, 4096, 0);
    e1_solo = 0; if (const char* v = getenv("LZ4F_MI355X_E1_SOLO")) e1_solo = (unsigned)atoi(v);
    if (on("LZ4F_MI355X_DETERMINISTIC")) e1_solo |= 1u;              // equal input -> equal bytes: one wave per workgroup parses, in order (see lz4f_mi355x_engine_set_deterministic)
    wait_ticks = 0; if (const char* v = getenv("LZ4F_MI355X_WAIT_TICKS")) { unsigned long long a = 0; if (sscanf(v, "%llu", &a) == 1) wait_ticks = a; }
    dblk_lds = (unsigned)num("LZ4F_MI355X_DBLK_LDS", 1, 150, 0) << 10;      // (development: fewer wave-per-block decoders per CU)
    recs_per_tile = (unsigned)num("LZ4F_MI355X_RECS_PER_TILE", 1, 16385, 0);
    hc_attempts = (unsigned)num("LZ4F_MI355X_HC_ATTEMPTS", 1, 65536, 0);      // (development: levels 3-12 search this many candidates per position)
    hc_lazy = (unsigned)num("LZ4F_MI355X_HC_LAZY", 1, 2, 0);
    seed = 2; if (const char* v = getenv("LZ4F_MI355X_SEED")) { unsigned a = 0; if (sscanf(v, "%u", &a) == 1 && a >= 1 && a <= 64) seed = a; }
}
namespace lz4f {
size_t new_engine(lz4f_mi355x_engine** out, int device, void* stream, bool borrow)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_last_error("no usable HIP device (hipGetDeviceCount: %s, count %d): liblz4f_mi355x has no CPU fallback", hipGetErrorString(e), n);
        return make_err(LZ4F_ERROR_GENERIC);
    }
    if (device < 0 || device >= n) { set_last_error("device %d out of range (%d devices)", device, n); return make_err(LZ4F_ERROR_GENERIC); }
    HIP_TRY(hipSetDevice(device));
    lz4f_mi355x_engine* en = new lz4f_mi355x_engine();
    en->device = device;
    en->sw.read();
    if (borrow) { en->stream = stream; en->own_stream = false; }
    else {
        hipStream_t s;
        hipError_t e2 = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e2 != hipSuccess) { delete en; set_last_error("hipStreamCreate failed: %s", hipGetErrorString(e2)); return make_err(LZ4F_ERROR_GENERIC); }
        en->stream = s; en->own_stream = true;
    }
    *out = en;
    return 0;
}

// ---- engines for the host-pointer entry points: a pool per process, not an engine per thread ----
// (A Haskell host's safe FFI calls land on arbitrary OS threads: engines owned by threads would be leaked with them - stream,
// pinned staging, device workspace.  A call borrows an idle engine of the wanted device, or makes one, and gives it back;
// lz4f_mi355x_release_engines() frees the idle ones, and so does the library's unload.)
namespace {
struct EnginePool {
    std::mutex mu;
    std::vector<lz4f_mi355x_engine*> idle;
    ~EnginePool() { drain(); }
    void drain()
    {
        std::vector<lz4f_mi355x_engine*> v;
        { std::lock_guard<std::mutex> g(mu); v.swap(idle); }
        for (auto* e : v) delete e;
    }
};
EnginePool& pool() { static EnginePool p; return p; }
}  // namespace

size_t acquire_engine(lz4f_mi355x_engine** out, int device)
{
    if (device < 0) device = selected_device();
    {
        EnginePool& p = pool();
        std::lock_guard<std::mutex> g(p.mu);
        for (size_t i = 0; i < p.idle.size(); i++)
            if (p.idle[i]->device == device) { *out = p.idle[i]; p.idle.erase(p.idle.begin() + i); return 0; }
    }
    return new_engine(out, device, nullptr, false);
}
void release_engine(lz4f_mi355x_engine* e)
{
    if (!e) return;
    EnginePool& p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    p.idle.push_back(e);
}
void release_idle_engines() { pool().drain(); }

}  // namespace lz4f

lz4f_mi355x_engine::~lz4f_mi355x_engine()
{
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize((hipStream_t)stream);
    desc.release(); seqcnt.release(); spx.release(); selfix.release(); selfcnt.release(); postab.release(); pdbuf.release(); tight.release();
    info.release(); recs.release(); e1_scratch.release(); walkbuf.release(); density.release(); ixtmp.release(); table.release(); blk_bytes.release(); res.release(); bad.release();
    d_in.release(); d_out.release(); bframes.release(); btable.release(); mframes.release(); mtable.release(); pctl.release(); split.release(); train.release(); cframes.release(); cblocks.release(); cchunks.release();
    h_in.release(); h_out.release(); h_small.release();
    for (int i = 0; i < 24; i++) if (ev[i]) (void)hipEventDestroy((hipEvent_t)ev[i]);
    if (aux_stream) { (void)hipStreamSynchronize((hipStream_t)aux_stream); (void)hipStreamDestroy((hipStream_t)aux_stream); }
    if (ev_fork) (void)hipEventDestroy((hipEvent_t)ev_fork);
    if (ev_join) (void)hipEventDestroy((hipEvent_t)ev_join);
    if (own_stream && stream) (void)hipStreamDestroy((hipStream_t)stream);
}

void lz4f_mi355x_engine::tick(int slot, bool end, void* on_stream)
{
    if (!timing) return;
    const int i = slot * 2 + (end ? 1 : 0);
    if (!ev[i]) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; ev[i] = e; }
    (void)hipEventRecord((hipEvent_t)ev[i], (hipStream_t)(on_stream ? on_stream : stream));
    if (end) ev_used[slot] = true;
}
bool lz4f_mi355x_engine::aux_ready()
{
    if (aux_stream && ev_fork && ev_join) return true;
    hipStream_t s; hipEvent_t a, b;
    if (!aux_stream) { if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return false; } aux_stream = s; }
    if (!ev_fork) { if (hipEventCreateWithFlags(&a, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; } ev_fork = a; }
    if (!ev_join) { if (hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; } ev_join = b; }
    return true;
}

size_t lz4f_mi355x_engine::sync()
{
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    // (work forked onto the second stream that the main stream never joined - a call that returned an error behind the fork: a caller that
    // frees its buffers after sync() must not race it)
    if (aux_pending && aux_stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)aux_stream)); aux_pending = false; }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// developer aid: cycle counters of workgroup 0 (LZ4F_MI355X_PROF=1), read back with lz4f_mi355x_debug_prof
static unsigned long long* g_prof = nullptr;
static unsigned long long* prof_buf()
{
    if (!g_prof) { if (hipMalloc(&g_prof, 1024) != hipSuccess) return nullptr; (void)hipMemset(g_prof, 0, 1024); (void)hipMemset(g_prof + 70, 0xFF, 8); (void)hipMemset(g_prof + 75, 0xFF, 8); }
    return g_prof;
}
extern "C" __attribute__((visibility("default"))) int lz4f_mi355x_debug_prof(unsigned long long* out128)
{
    if (!prof_buf()) return 1;
    (void)hipDeviceSynchronize();
    const int rc = hipMemcpy(out128, g_prof, 1024, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
#ifdef DB_PROF
    { unsigned long long z[32] = {0}; (void)hipMemcpyFromSymbol(out128 + 96, HIP_SYMBOL(lz4f::g_dbprof), sizeof(z)); (void)hipMemcpyToSymbol(HIP_SYMBOL(lz4f::g_dbprof), z, sizeof(z)); }
#endif
    (void)hipMemset(g_prof, 0, 1024); (void)hipMemset(g_prof + 70, 0xFF, 8); (void)hipMemset(g_prof + 75, 0xFF, 8);      // (the grid-wide words accumulate: start again)
    return rc;
}

static uint32_t device_cus(int device)
{
    static int cus[64];                                                  // (0: not asked yet; a benign race: every thread stores the same number)
    const unsigned d = (unsigned)device % 64;
    if (!cus[d]) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v < 1) v = 256; cus[d] = v; }
    return (uint32_t)cus[d];
}

// ------------------------------------------------------------------------------------------------
// encode: a plan made from the call alone, then one function per stage (launch_compress, behind them, runs them in order)

// How `payload` bytes fall into blocks, and a block into the chunks of passes E1, S and E2.  The public sizing calls (a caller sizes
// its buffers by them) and the engine (it fills them) both go by these.
struct EncShape { uint32_t chunk, chunks_per_block; uint64_t n_blocks; };
static EncShape enc_shape(uint64_t payload, uint32_t block_size)
{
    const uint32_t chunk = pick_chunk_size(block_size);
    return EncShape{chunk, block_size / chunk, (payload + block_size - 1) / block_size};
}
// the sequence index: its fixed part and room for one sequence per 64 bytes of input on average (ix_typical_entries)
static size_t index_capacity(uint64_t payload, const EncShape& s)
{
    return ix_entries_at((uint32_t)s.n_blocks, s.chunks_per_block) + ix_typical_entries(payload, (uint32_t)(s.n_blocks * s.chunks_per_block)) * sizeof(IxEntry);
}

// The record pool of one compress call, in records: `per_tile` a 64 KiB tile on average (0 = the default, 12288: a sequence per 5.3 input
// bytes - the densest input of the tests, Zipf text, needs more than 8192 per tile; the bench input one per 2000), never less than 64 tiles' worst case
// (small calls are sized for the worst case outright) and never more than the worst case.  LZ4F_MI355X_RECS_PER_TILE=16385 is the worst
// case for every tile; a caller that knows its data is sparse sets it low (1024: 0.13 bytes of workspace per input byte).
static uint64_t rec_pool_records(uint32_t n_chunks, uint32_t max_rec_per_chunk, unsigned per_tile)
{
    const uint64_t worst = (uint64_t)(n_chunks + 1) * max_rec_per_chunk;
    uint64_t want = (uint64_t)(n_chunks + 1) * (per_tile ? per_tile : 12288u);
    if (want < 64ull * max_rec_per_chunk) want = 64ull * max_rec_per_chunk;
    if (want > worst) want = worst;
    if (want > 0xFFFFFFF0ull) want = 0xFFFFFFF0ull;                      // (a list's place is a 32-bit record number)
    return want;
}

// levels 3-12: the chain candidates a search looks at and the lazy parse's depth - the level's (hc_level), unless a development switch
// sets one
static HcLevel hc_level_of(int level, const lz4f_mi355x_engine::Switches& sw)
{
    const HcLevel hl = hc_level(level);
    return HcLevel{sw.hc_attempts ? sw.hc_attempts : hl.attempts, sw.hc_lazy ? sw.hc_lazy : hl.lazy};
}

struct lz4f_mi355x_engine::EncodePlan {
    bool too_large;                  // more chunks than a 32-bit count holds: the call is refused, nothing else here is filled in
    EncGeom g;                       // what every kernel of the call takes
    enum Finder { E1_SHARED, E1_SOLO, HASH_CHAIN } finder;      // pass E1 (encode.cuh), its deterministic form (encode_solo.cuh), levels 3-12 (encode_hc.cuh)
    uint32_t e1_wgs;                 // the shared pass E1's workgroups, each with a run of g.tiles_per_wg tiles
    bool layout_small, e2_split;     // a few blocks: one layout launch instead of three; few chunks: the four waves of an emit workgroup share a chunk
    bool xxh_lane4;                  // few big blocks: a block checksum's four accumulators as four lanes
    bool inband;                     // the index is made in the engine's own buffer and copied into a trailer behind the frame
    size_t index_cap;                // bytes of the sequence index: the caller's, or (in-band) of the engine's own buffer
    size_t info_bytes, recs_bytes, blk_bytes, table_bytes, res_bytes, e1_scratch_bytes, ixtmp_bytes;      // the workspaces (table: when the caller brings none; ixtmp: in-band)
};

lz4f_mi355x_engine::EncodePlan lz4f_mi355x_engine::encode_plan(const CompressJob& j, const Switches& sw, uint32_t cus, bool inband, size_t index_cap)
{
    EncodePlan p; memset(&p, 0, sizeof(p));
    EncGeom& g = p.g;
    const uint64_t payload = j.src_size - j.first_off;
    const EncShape s = enc_shape(payload, j.block_size);
    if (s.n_blocks > 0x7FFFFFFFull / s.chunks_per_block) { p.too_large = true; return p; }
    g.src_size = j.src_size; g.first_off = j.first_off; g.write_endmark = j.endmark ? (j.content_checksum ? 2 : 1) : 0;
    g.block_size = j.block_size; g.chunk_size = s.chunk; g.chunks_per_block = s.chunks_per_block;
    g.n_blocks = (uint32_t)s.n_blocks; g.n_chunks = g.n_blocks * g.chunks_per_block;
    g.linked = j.linked; g.block_checksum = j.block_checksum;
    g.header_size = j.header_size; memcpy(g.header, j.header, j.header_size);
    g.max_rec_per_chunk = g.chunk_size / 4 + 1;
    g.seed_stride = sw.seed;
    // deterministic mode: a wave per chunk with a table of its own (encode_solo.cuh) - nothing shared, nothing that depends on timing.
    // (e1_solo bit 2: the shared kernel with one wave per workgroup parsing, the mode's form until round 4 - kept for comparison)
    // levels 3-12: the hash-chain finder, a workgroup per chunk (encode_hc.cuh) - deterministic too.
    const bool hc = j.level >= 3;
    p.finder = hc ? EncodePlan::HASH_CHAIN : ((sw.e1_solo & 1u) && !(sw.e1_solo & 4u)) ? EncodePlan::E1_SOLO : EncodePlan::E1_SHARED;
    if (hc) { const HcLevel hl = hc_level_of(j.level, sw); g.hc_attempts = hl.attempts; g.hc_lazy = hl.lazy; }
    // (deterministic mode: the worst case for every tile - which tiles a short pool turns away is a matter of which workgroup's merge
    // gets to the bump pointer first, and "equal input, equal bytes" must not hang on that: 2 bytes of workspace per input byte)
    // (levels 3-12 likewise: their output is a function of the input alone, so a chunk's list has a place of its own, encode_hc.cuh)
    g.rec_pool = rec_pool_records(g.n_chunks, g.max_rec_per_chunk, ((sw.e1_solo & 1u) || hc) ? 16385u : sw.recs_per_tile);
    if (g.n_chunks) {
        // a workgroup (one per CU: ~150 KiB of LDS) takes a run of consecutive 64 KiB tiles.  At most 1024 workgroups (each
        // has its slice lists in `e1_scratch`).  Round 4: as many workgroups as there are CUs where the input has fewer than 64 tiles
        // for each, runs of 64 tiles from there on - a run's first tile pays for the 64 KiB of history in front of it, for seeding the
        // table with them and for not knowing the data's density yet, so fewer, longer runs win until the CUs run out of work:
        // tools/e1_run_sweep.py, tiles per workgroup 1024-wide rule -> this one: 64 MiB 0.132 -> 0.065 ms (ratio 1.9154 -> 1.9425),
        // 256 MiB 0.256 -> 0.187, 1 GiB 0.722 -> 0.647, 2 GiB 1.342 -> 1.228; 4 GiB and beyond as before (64 tiles, 1024 workgroups).
        uint32_t run = g.n_chunks / cus; run = run < 1 ? 1 : run > 64 ? 64 : run;
        if ((g.n_chunks + run - 1) / run > 1024) run = (g.n_chunks + 1023) / 1024;
        if (sw.e1_run) run = sw.e1_run;
        g.tiles_per_wg = run;
        g.e1_solo = sw.e1_solo;
        p.e1_wgs = (g.n_chunks + run - 1) / run;
        p.e1_scratch_bytes = (size_t)p.e1_wgs * 2 * E1_NSLICE * E1_REC_PER_SLICE * 8 + 2048;      // (the last 2048: E1_DEBUG's counters)
    }
    p.layout_small = g.n_blocks <= LAYOUT_SMALL_BLOCKS && g.n_chunks <= LAYOUT_SMALL_CHUNKS; p.e2_split = g.n_chunks <= 512;      // (both: the streaming API's one block per call)
    p.xxh_lane4 = g.n_blocks < XXH_LANE4_BELOW;
    p.inband = inband;
    p.index_cap = inband ? index_capacity(payload, s) + 64 : index_cap;
    p.ixtmp_bytes = inband ? p.index_cap + 64 : 0;
    p.info_bytes = (size_t)(g.n_chunks + 1) * sizeof(ChunkInfo); p.recs_bytes = (size_t)(rec_pool_at(g.n_chunks) + g.rec_pool) * 8;
    p.blk_bytes = (size_t)(g.n_blocks + 1) * 4; p.table_bytes = (size_t)(g.n_blocks + 1) * sizeof(BlockOut);
    p.res_bytes = sizeof(ResultRec) + sizeof(TrailerPlan) + 64;                                   // (the in-band trailer's plan rides behind the record)
    return p;
}

#ifdef E1_DEBUG
// developer aid (-DE1_DEBUG): pass E1's counters, behind the workgroups' slice lists in e1_scratch
static void e1_debug_dump(hipStream_t st, const uint8_t* counters)
{
    unsigned long long d[256]; if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(d, counters, 2048, hipMemcpyDeviceToHost) == hipSuccess) {
                for (int w = 0; w < 16; w += 5) { unsigned long long* x = d + 16 + w * 8; if (x[6]) fprintf(stderr, "E1 wave %d: per tile cycles: merge %llu parse %llu waitB1 %llu dma-issue %llu dma-wait %llu waitB2 %llu (%llu tiles)\n", w, x[0]/x[6], x[1]/x[6], x[2]/x[6], x[3]/x[6], x[4]/x[6], x[5]/x[6], x[6]); unsigned long long* f = d + 160 + w * 6; fprintf(stderr, "   parse: dequeue %llu cycles x %llu, probe step %llu cycles x %llu, hit %llu cycles x %llu (per tile)\n", f[3] ? f[0]/f[3] : 0, f[3]/x[6], f[4] ? f[1]/f[4] : 0, f[4]/x[6], f[5] ? f[2]/f[5] : 0, f[5]/x[6]); }
                fprintf(stderr, "E1 dense passes (workgroup 0): %llu, matches taken %llu, positions advanced %llu; one-match steps because: hit in B %llu, mode not dense %llu, step != 1 %llu, first match long %llu\n", d[13], d[14], d[15], d[4], d[5], d[6], d[7]);
                fprintf(stderr, "E1 debug: bounds hit: dequeue %llu, probe %llu, backward %llu, forward %llu; probe ip/last %llx step/slice %llx; back room/nb %llx; fwd mp/fw %llx end_lim/d %llx\n", d[0], d[1], d[2], d[3], d[8], d[9], d[10], d[11], d[12]); }
}
#endif

// Stage 1: the workspaces, each ensured once.  own_table: the caller brought no block table.
size_t lz4f_mi355x_engine::enc_workspaces(const EncodePlan& p, bool own_table)
{
    if (ixtmp.ensure(p.ixtmp_bytes) || res.ensure(p.res_bytes) || info.ensure(p.info_bytes) || recs.ensure(p.recs_bytes) || blk_bytes.ensure(p.blk_bytes) ||
        (own_table && table.ensure(p.table_bytes)) || e1_scratch.ensure(p.e1_scratch_bytes))
        return make_err(LZ4F_ERROR_allocation_failed);
    return 0;
}

// Stage 2: the match finder - every chunk's sequences as records in the pool
size_t lz4f_mi355x_engine::enc_find(const CompressJob& j, const EncodePlan& p)
{
    hipStream_t st = (hipStream_t)stream; const EncGeom& g = p.g;
#ifdef E1_DEBUG
    uint8_t* const counters = (uint8_t*)e1_scratch.p + p.e1_scratch_bytes - 2048;
    (void)hipMemsetAsync(counters, 0, 2048, st);
#endif
    // (the pool's bump pointer and its count of tiles turned away: every call's scan leaves them at zero for the next; zeroed here when the
    // workspace is new, or when a call before this one may not have got as far as its scan)
    if (recs_ctl_clean != recs.p) { HIP_TRY(hipMemsetAsync(recs.p, 0, 64, st)); }
    recs_ctl_clean = nullptr;
    if (p.finder == EncodePlan::HASH_CHAIN)
        hipLaunchKernelGGL(k_find_matches_hc, dim3(g.n_chunks), dim3(64 * HC_WAVES), 0, st, j.d_src, g, (ChunkInfo*)info.p, (uint64_t*)recs.p);
    else if (p.finder == EncodePlan::E1_SOLO)
        hipLaunchKernelGGL((k_find_matches_solo<1>), dim3(g.n_chunks), dim3(64), 0, st, j.d_src, g, (ChunkInfo*)info.p, (uint64_t*)recs.p);
    else
        hipLaunchKernelGGL(k_find_matches, dim3(p.e1_wgs), dim3(64 * E1_WAVES), 0, st, j.d_src, g, (ChunkInfo*)info.p, (uint64_t*)recs.p, (uint64_t*)e1_scratch.p);
    if (sw.e1_sync) (void)hipStreamSynchronize(st);
#ifdef E1_DEBUG
    e1_debug_dump(st, counters);
#endif
    return 0;
}

// Stage 3: the layout - every block's and chunk's place in the frame, the header, the result record - and the sequence index
void lz4f_mi355x_engine::enc_layout(const EncodePlan& p, uint8_t* d_dst, uint64_t dst_cap, ResultRec* rec, BlockOut* tbl, void* d_index)
{
    constexpr int W = 4;
    hipStream_t st = (hipStream_t)stream; const EncGeom& g = p.g;
    if (p.layout_small)
        hipLaunchKernelGGL(k_layout_small, dim3(1), dim3(1024), 0, st, g, (ChunkInfo*)info.p, tbl, (uint32_t*)blk_bytes.p, d_dst, dst_cap, rec, (const uint64_t*)recs.p);
    else {
        if (g.n_blocks) hipLaunchKernelGGL((k_layout_blocks<W>), dim3((g.n_blocks + W - 1) / W), dim3(64 * W), 0, st, g, (ChunkInfo*)info.p, tbl, (uint32_t*)blk_bytes.p);
        hipLaunchKernelGGL(k_layout_scan, dim3(1), dim3(1024), 0, st, g, tbl, (const uint32_t*)blk_bytes.p, d_dst, dst_cap, rec, (const uint64_t*)recs.p);
        if (g.n_chunks) hipLaunchKernelGGL(k_layout_chunks, dim3((g.n_chunks + 255) / 256), dim3(256), 0, st, g, (ChunkInfo*)info.p, (const BlockOut*)tbl, d_dst, (const ResultRec*)rec);
    }
    if (g.n_chunks) recs_ctl_clean = recs.p;                                  // (the scan is enqueued: it leaves the pool's control words at zero)
    if (d_index) {                                                            // sequence index for the indexed decoder
        if (g.n_blocks) hipLaunchKernelGGL((k_index_blocks<W>), dim3((g.n_blocks + W - 1) / W), dim3(64 * W), 0, st, g, (const ChunkInfo*)info.p, (const BlockOut*)tbl, (const ResultRec*)rec, d_index, (uint64_t)p.index_cap);
        hipLaunchKernelGGL(k_build_index, dim3(1), dim3(1024), 0, st, g, (const ChunkInfo*)info.p, (const BlockOut*)tbl, (const ResultRec*)rec, d_index, (uint64_t)p.index_cap, 1u);
    }
}

// Stage 4: the emit - the chunks' records and literals become the blocks' bytes - and the block checksums behind it
void lz4f_mi355x_engine::enc_emit(const CompressJob& j, const EncodePlan& p, uint8_t* d_dst, const ResultRec* rec, BlockOut* tbl, void* d_index)
{
    constexpr int W = 4;
    hipStream_t st = (hipStream_t)stream; const EncGeom& g = p.g;
    tick(2, false);
    if (p.e2_split)
        hipLaunchKernelGGL((k_emit_gather<W, true>), dim3(g.n_chunks), dim3(64 * W), 0, st, j.d_src, g, (const ChunkInfo*)info.p,
                           (const uint64_t*)recs.p, d_dst, (const BlockOut*)tbl, d_index);
    else
        hipLaunchKernelGGL((k_emit_gather<W, false>), dim3((g.n_chunks + W - 1) / W), dim3(64 * W), 0, st, j.d_src, g, (const ChunkInfo*)info.p,
                           (const uint64_t*)recs.p, d_dst, (const BlockOut*)tbl, d_index);
    tick(2, true);
    if (!j.block_checksum) return;
    tick(3, false);
    if (p.xxh_lane4)                                                   // (lane4_xxh32)
        hipLaunchKernelGGL((k_xxh32_blocks4<1>), dim3(g.n_blocks), dim3(64), XXH_SPREAD_LDS, st, d_dst, tbl, rec, g.n_blocks, 0u, (FinishVerdict*)nullptr);
    else
        hipLaunchKernelGGL((k_xxh32_blocks<W>), dim3((g.n_blocks + W - 1) / W), dim3(64 * W), 0, st, d_dst, tbl, rec, g.n_blocks, 0u, (FinishVerdict*)nullptr);
    tick(3, true);
}

// Stage 5: what ends a frame - the content checksum behind the EndMark, and the in-band trailer: block list and index behind the frame
void lz4f_mi355x_engine::enc_tail(const CompressJob& j, const EncodePlan& p, uint8_t* d_dst, uint64_t dst_cap, ResultRec* rec, const BlockOut* tbl, const void* d_index)
{
    hipStream_t st = (hipStream_t)stream; const EncGeom& g = p.g;
    if (j.endmark && j.content_checksum)                              // (one chain over the whole input: see k_xxh32_content for what that costs)
        hipLaunchKernelGGL(k_xxh32_content, dim3(1), dim3(64), 0, st, j.d_src + j.first_off, (uint64_t)(j.src_size - j.first_off), d_dst, rec, 0u);
    if (p.inband && g.n_blocks) {
        TrailerPlan* plan = (TrailerPlan*)((uint8_t*)res.p + sizeof(ResultRec) + 32);
        hipLaunchKernelGGL(k_trailer_plan, dim3(1), dim3(64), 0, st, d_dst, dst_cap, rec, g.n_blocks, d_index,
                           (uint64_t)ix_entries_at(g.n_blocks, g.chunks_per_block), plan);
        hipLaunchKernelGGL(k_trailer_copy, dim3(256), dim3(256), 0, st, d_dst, (const TrailerPlan*)plan, tbl, g.n_blocks, d_index);
    }
}

lz4f_mi355x_engine::CompressJob lz4f_mi355x_engine::make_compress_job(const uint8_t* d_src, uint64_t src_size, uint64_t first_off, uint32_t block_size,
                                                                      bool linked, bool block_checksum, int level, const LZ4F_preferences_t* frame)
{
    CompressJob j; memset(&j, 0, sizeof(j));
    j.d_src = d_src; j.src_size = src_size; j.first_off = first_off; j.block_size = block_size;
    j.linked = linked; j.block_checksum = block_checksum; j.level = level;
    if (frame) { j.endmark = true; j.content_checksum = frame->frameInfo.contentChecksumFlag != 0; j.header_size = (uint32_t)write_frame_header(j.header, *frame); }
    return j;
}

size_t lz4f_mi355x_engine::launch_compress(const CompressJob& j, uint8_t* d_dst, uint64_t dst_cap,
                                           lz4f_mi355x_result* d_res, lz4f_mi355x_block* d_table, void* d_index, size_t index_cap)
{   // in-band: the index is made in the engine's own buffer and copied, with the block list, into a skippable frame behind the
    // LZ4 frame (frame_dev.cuh: the trailer)
    const bool inband = d_index == nullptr && index_cap == LZ4F_MI355X_INBAND;
    HIP_TRY(hipSetDevice(device));                     // (before anything is allocated: the caller's current device may be another one)
    const EncodePlan p = encode_plan(j, sw, device_cus(device), inband, index_cap);
    if (inband && ((uintptr_t)d_dst & 15) != 0) { set_last_error("in-band index: the frame buffer must be 16-byte aligned"); return make_err(LZ4F_ERROR_GENERIC); }
    if (p.too_large) { set_last_error("input too large for one call"); return make_err(LZ4F_ERROR_srcSize_tooLarge); }
    if (size_t e = enc_workspaces(p, !d_table)) return e;
    if (inband) d_index = ixtmp.p;
    BlockOut* tbl = (BlockOut*)(d_table ? d_table : table.p);
    ResultRec* r = (ResultRec*)(d_res ? d_res : res.p);
    for (int i = 0; i < 4; i++) ev_used[i] = false;
    ev_used[10] = false;
    tick(10, false);
    if (p.g.n_chunks) {
        tick(0, false);
        if (size_t e = enc_find(j, p)) return e;
        tick(0, true);
    }
    tick(1, false);
    enc_layout(p, d_dst, dst_cap, r, tbl, d_index);
    tick(1, true);
    if (p.g.n_chunks) enc_emit(j, p, d_dst, r, tbl, d_index);
    enc_tail(j, p, d_dst, dst_cap, r, tbl, d_index);
    tick(10, true);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// decode: a plan made from the call alone, then one function per stage (launch_decompress, at the end, runs them in order)
lz4f_mi355x_engine::DecodePlan lz4f_mi355x_engine::decode_plan(const DecompressJob& j, const Switches& sw, uint32_t cus)
{
    DecodePlan p;
    p.given = j.d_table || j.table_in_place || j.table_direct;
    p.n_max = p.given ? j.n_blocks : j.max_blocks;
    p.begin_small = p.given && p.n_max <= 256;                       // (the streaming API's one block per call: one launch for the record, the verdict words and the table check)
    const bool hinted = j.hint_list && j.hint_n <= p.n_max;
    // frames of many small blocks: the size words are found in parallel (frame_dev.cuh); k_walk_frame behind it returns at
    // once when that has delivered, and walks the list itself otherwise (big blocks: a few hundred hops, and one in 2^9
    // byte positions would be a candidate)
    if (p.given) p.walk = DecodePlan::WALK_NONE;
    else if (hinted) p.walk = DecodePlan::WALK_TRAILER;
    else if (j.block_size <= (256u << 10) && j.frame_cap >= (1u << 20) && !sw.serial_walk) p.walk = DecodePlan::WALK_PARALLEL;
    else if (j.block_size > (256u << 10) && j.frame_cap >= (size_t)192 * j.block_size && !sw.serial_walk) p.walk = DecodePlan::WALK_SEEDED;      // (~0.15 ms whatever the frame: pays from ~330 blocks of half their size on)
    else p.walk = DecodePlan::WALK_SERIAL;
    // large blocks / linked frames: fused parse+copy workgroups ('f'); small independent blocks: one wave per block ('1')
    p.mode = sw.decode_mode ? sw.decode_mode : (j.linked || j.block_size >= (256u << 10)) ? 'f' : '1';
    // (an index out of the frame's trailer brings its counts in the footer - no read - and its frame is one call's work: every block but the last is full,
    // so the table the list check writes has every block's place in the output, which is what a linked frame's indexed decode needs; if a trailer lies about
    // that the descriptors do not tile the blocks and the generic kernels take the frame)
    p.ix_by_trailer = j.d_index && j.ix_seqs && hinted;
    // no index to go by: a linked frame's is made by a lane per block, big independent blocks' from stitched stretches (dec_self_index)
    p.self_index = !sw.no_selfindex && (j.linked ? j.hist0 <= 65536 && p.n_max >= 2 : j.block_size >= (256u << 10) && j.block_size <= (4u << 20) && !sw.no_spx);
    // (an index out of the frame's trailer is laid out for the block count the trailer names; the table and the generic
    // kernels keep the caller's upper bound - if the walk finds another count, the index is dropped on the device)
    p.n_ix = hinted ? j.hint_n : p.n_max;
    // a linked frame is one chain: one workgroup with the 64 KiB window in LDS; frames with short (flushed) blocks
    // set the flag and are decoded by the generic kernel launched right behind (it returns at once otherwise)
    // (one block of a linked frame - what the streaming functions hand over per call: the window kernel is built for whole frames
    // and takes 180-210 us for a single 64 KiB block; the fused workgroup takes it directly)
    p.windowed = j.linked && j.dst_cap < 0xFFF00000ull && !sw.no_window && !(p.n_max == 1 && p.given);
    // more blocks than the machine has 8-wave workgroup slots: the 4-wave shape keeps twice as many in flight
    p.small = !j.linked && j.block_size <= (1u << 20);
    // Few big blocks: a wave per block leaves the machine idle and waits out every trip to memory (13-15 GiB/s for a GiB in 4 MiB blocks);
    // a workgroup per block with the block's window in LDS and its waves taking the payload in turns (decode_relay.cuh) is three times
    // as fast per block - but it has a CU to itself, so from ~3 blocks per CU on the waves win again (8 GiB in 4 MiB blocks: 90 GiB/s).
    p.relay = j.block_size > 65536u && sw.dense_mode != 2 && (sw.dense_mode == 1 || p.n_max <= 3u * cus);
    // (linked frames of small blocks: a workgroup takes a group of consecutive blocks - see k_copy_indexed)
    // (a group is 1 MiB of blocks where that fills the machine - 1024 workgroups of the 4-wave shape are half of its wave slots - and less for
    // smaller frames: LZ4F_MI355X_GROUP_KIB sets it)
    const uint32_t group_bytes = sw.group_kib ? sw.group_kib << 10 : ((uint64_t)p.n_ix * j.block_size <= (2ull << 30) ? (512u << 10) : (1u << 20));      // (1 GiB: 512 KiB 0.509 ms, 1 MiB 0.541, 256 KiB 0.788, 2 MiB 0.778)
    p.group = (j.linked && j.block_size < group_bytes && !sw.no_groups) ? group_bytes / j.block_size : 1u;
    // (how long a group of a linked frame waits for the one in front: half a second plus 20 ticks of the 100 MHz clock per
    // output byte - 5 MB/s, a fifth of the slowest chain measured (text, linked, 27 MB/s); LZ4F_MI355X_WAIT_TICKS overrides)
    p.wait_ticks = sw.wait_ticks ? sw.wait_ticks : 50000000ull + 20ull * p.n_ix * j.block_size;
    return p;
}
lz4f_mi355x_engine::IxRoute lz4f_mi355x_engine::ix_route(const DecompressJob& j, const Switches& sw, uint32_t n_ix, uint32_t ix_seqs)
{
    IxRoute r;
    const uint64_t span = (uint64_t)n_ix * j.block_size;            // (the last block may be short)
    // (pointer doubling does ~12 GiB/s on text whatever the framing; hop by hop it is 1.3 GiB/s, which only pays where
    // there is no block-level parallelism - linked frames; independent blocks then stay with the copier workgroups, 4.8 GiB/s)
    r.doubling = ((uint64_t)ix_seqs * 48 > span || sw.trace_always) && span <= IXP_MAX_SPAN && !sw.no_doubling;      // (short sequences: worth the tracer's scratch)
    // Independent blocks that are not dense (no tracer on offer): ONE kernel - the copy workgroup's first wave parses its block's
    // runs and resolves direct matches while the copiers move bytes (decode_indexed.cuh: k_copy_selffed)
    r.selffed = !j.linked && !sw.no_selffeed && !sw.no_resolve && !sw.trace_always && !r.doubling;
    const bool trace_can = !sw.no_trace && !sw.no_resolve && (j.block_size & 63u) == 0;
    r.gate = !trace_can ? 0u : sw.trace_always ? 2u : (j.linked || r.doubling) ? 1u : 0u;
    return r;
}
// a DevBuf carved into arrays: take() them in order, ensure(), then at()
struct Carve {
    DevBuf& buf;
    size_t end = 0;
    size_t take(size_t bytes, size_t align = 1) { const size_t at = (end + align - 1) & ~(align - 1); end = at + bytes; return at; }
    int ensure() { return buf.ensure(end); }
    template <typename T> T* at(size_t off) const { return (T*)((uint8_t*)buf.p + off); }
};
// developer aid (LZ4F_MI355X_PROF): wait for the stream, then copy n bytes of the device's counters back
static bool prof_read(hipStream_t st, void* to, const void* from, size_t n) { return hipStreamSynchronize(st) == hipSuccess && hipMemcpy(to, from, n, hipMemcpyDeviceToHost) == hipSuccess; }

// Stage 1: the block table - the caller's, checked, or found by walking the frame's size words - and the finishing kernels' verdict words.
size_t lz4f_mi355x_engine::dec_table(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut** tbl_out, uint32_t* path)
{
    hipStream_t st = (hipStream_t)stream; const uint32_t n_max = p.n_max;
    // a caller-supplied table is worked on in a copy (decode overwrites dst_size); table_direct: the engine's own staging copy, used where it lies
    BlockOut* tbl = (BlockOut*)j.table_direct;
    if (!tbl) { if (table.ensure((size_t)(n_max + 1) * sizeof(BlockOut))) return make_err(LZ4F_ERROR_allocation_failed); tbl = (BlockOut*)table.p; }
    if (p.given) {
        if (!j.table_in_place && !j.table_direct)
            HIP_TRY(hipMemcpyAsync(tbl, j.d_table, (size_t)n_max * sizeof(BlockOut), hipMemcpyDeviceToDevice, st));
        if (p.begin_small)
            hipLaunchKernelGGL(k_begin_table_small, dim3(1), dim3(256), 0, st, (const BlockOut*)tbl, n_max, (uint64_t)j.frame_cap, (uint64_t)j.dst_cap,
                               j.block_size, j.block_checksum ? 1u : 0u, j.linked ? 1u : 0u, res, (FinishVerdict*)bad.p);
        else {
            hipLaunchKernelGGL(k_init_result, dim3(1), dim3(64), 0, st, res, n_max, 0u);
            if (n_max) hipLaunchKernelGGL(k_check_table, dim3(std::min<uint32_t>((n_max + 255) / 256, 1024u)), dim3(256), 0, st, (const BlockOut*)tbl, n_max, (uint64_t)j.frame_cap, (uint64_t)j.dst_cap,
                                          j.block_size, j.block_checksum ? 1u : 0u, j.linked ? 1u : 0u, res);
        }
        *path |= LZ4F_MI355X_PATH_TABLE_GIVEN;
    } else {
        tick(4, false);
        // the list walks: each finds where the size words should be in its own way, then the same two kernels check the list link by link
        const size_t list_cap = (size_t)n_max + 1024;                     // (the parallel and the seeded walk's list)
        uint32_t lgrid = std::min<uint32_t>((uint32_t)((list_cap + 255) / 256), 4096u);
        WalkState* ws = nullptr; const uint64_t* list = nullptr;
        if (p.walk == DecodePlan::WALK_TRAILER) {
            // the frame's own trailer says where the size words are: checked link by link like the parallel walk's candidates
            if (walkbuf.ensure(256)) return make_err(LZ4F_ERROR_allocation_failed);
            ws = (WalkState*)walkbuf.p;
            hipLaunchKernelGGL(k_walk_head, dim3(1), dim3(64), 0, st, j.d_frame, j.frame_cap, ws, j.hint_n);
            list = j.hint_list;
            lgrid = std::min<uint32_t>((j.hint_n + 255) / 256, 4096u);
            *path |= LZ4F_MI355X_PATH_TRAILER;
        } else if (p.walk == DecodePlan::WALK_PARALLEL) {
            const uint32_t n_chunks = (uint32_t)((j.frame_cap + WK_CHUNK - 1) / WK_CHUNK);
            Carve wb{walkbuf};
            const size_t at_state = wb.take(256), at_chunks = wb.take((size_t)n_chunks * sizeof(WalkChunk)), at_list = wb.take(list_cap * 8), at_list2 = wb.take(list_cap * 8), at_mark = wb.take(list_cap * 4);
            if (wb.ensure()) return make_err(LZ4F_ERROR_allocation_failed);
            ws = wb.at<WalkState>(at_state);
            WalkChunk* ch = wb.at<WalkChunk>(at_chunks);
            uint64_t* list1 = wb.at<uint64_t>(at_list);
            uint64_t* list2 = wb.at<uint64_t>(at_list2);
            uint32_t* mark = wb.at<uint32_t>(at_mark);
            HIP_TRY(hipMemsetAsync(mark, 0, list_cap * 4, st));
            hipLaunchKernelGGL(k_walk_head, dim3(1), dim3(64), 0, st, j.d_frame, j.frame_cap, ws);
            hipLaunchKernelGGL(k_walk_cand, dim3(n_chunks), dim3(256), 0, st, j.d_frame, j.frame_cap, (const WalkState*)ws, ch);
            hipLaunchKernelGGL(k_walk_order, dim3(1), dim3(1024), 0, st, ch, n_chunks, ws, list1, (uint32_t)list_cap);
            hipLaunchKernelGGL(k_walk_mark, dim3(lgrid), dim3(256), 0, st, j.d_frame, j.frame_cap, (const WalkState*)ws, (const uint64_t*)list1, mark);
            hipLaunchKernelGGL(k_walk_filter, dim3(1), dim3(1024), 0, st, ws, (const uint64_t*)list1, (const uint32_t*)mark, list2);
            list = list2;
            *path |= LZ4F_MI355X_PATH_PARALLEL_WALK;
        } else if (p.walk == DecodePlan::WALK_SEEDED) {
            // big blocks: seeds found in parallel, a lane per seed walking to the next one (frame_dev.cuh); the list is checked link by
            // link like the small blocks' candidates, and k_walk_frame behind walks the frame itself if it is not the chain
            Carve wb{walkbuf};
            const size_t at_state = wb.take(256), at_seeds = wb.take((WK_SEEDS + 1) * 8), at_list = wb.take(list_cap * 8);
            if (wb.ensure()) return make_err(LZ4F_ERROR_allocation_failed);
            ws = wb.at<WalkState>(at_state);
            unsigned long long* seeds = wb.at<unsigned long long>(at_seeds);
            HIP_TRY(hipMemsetAsync(seeds, 0xFF, (WK_SEEDS + 1) * 8, st));
            uint64_t* list1 = wb.at<uint64_t>(at_list);
            hipLaunchKernelGGL(k_walk_head, dim3(1), dim3(64), 0, st, j.d_frame, j.frame_cap, ws);
            hipLaunchKernelGGL(k_walk_seeds, dim3(WK_SEEDS * wk_seed_pieces(j.block_size)), dim3(256), 0, st, j.d_frame, j.frame_cap, (const WalkState*)ws, seeds);
            hipLaunchKernelGGL(k_walk_chains, dim3(1), dim3(WK_SEEDS), 0, st, j.d_frame, j.frame_cap, ws, (const unsigned long long*)seeds, list1, (uint32_t)std::min<size_t>(list_cap, 0xFFFFFFFFu));
            list = list1;
            *path |= LZ4F_MI355X_PATH_PARALLEL_WALK;
        }
        if (list) {
            hipLaunchKernelGGL(k_walk_link, dim3(lgrid), dim3(256), 0, st, j.d_frame, j.frame_cap, j.dst_cap, ws, list, tbl, n_max);
            hipLaunchKernelGGL(k_walk_verdict, dim3(1), dim3(64), 0, st, j.d_frame, j.frame_cap, j.dst_cap, ws, list, n_max, res, p.walk == DecodePlan::WALK_TRAILER ? 1u : 0u);
            WalkState h;
            if (sw.prof && p.walk == DecodePlan::WALK_PARALLEL && prof_read(st, &h, ws, sizeof(h))) fprintf(stderr, "parallel walk: done %u overflow %u candidates %u first_end %u first_break %u (header ok %u, hsize %u, block %u)\n", h.done, h.overflow, h.total, h.first_end, h.first_break, h.head_ok, h.hsize, h.bs);
            if (sw.prof && p.walk == DecodePlan::WALK_SEEDED && prof_read(st, &h, ws, sizeof(h))) fprintf(stderr, "seeded walk: done %u overflow %u entries %u first_end %u first_break %u\n", h.done, h.overflow, h.total, h.first_end, h.first_break);
        }
        hipLaunchKernelGGL(k_walk_frame, dim3(1), dim3(64), 0, st, j.d_frame, j.frame_cap, j.dst_cap, tbl, n_max, res, list ? (const uint32_t*)&ws->done : nullptr);
        tick(4, true);
    }
    if (!p.begin_small) {                                              // (k_begin_table_small set them)
        HIP_TRY(hipMemsetAsync(bad.p, 0xFF, FINISH_ONES, st));       // the two "first block that ..." words
        HIP_TRY(hipMemsetAsync((uint8_t*)bad.p + FINISH_ONES, 0, sizeof(FinishVerdict) - FINISH_ONES, st));
    }
    *tbl_out = tbl;
    return 0;
}

// Stage 2: the block checksums.  The verification only reads the payloads, and so do the decode kernels: it runs beside them on the
// engine's second stream (forked here, joined in front of k_finish_check, which reads its verdict).  A 4 MiB block is one serial chain
// for one wave (~2 ms) whatever else the GPU does, so side by side the two cost max(2.0, decode) instead of the sum.  The one-wave
// workgroups then ask for 12 KiB of LDS instead of 36 (they would not fit beside four decode workgroups per CU).
size_t lz4f_mi355x_engine::dec_checksums(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut* tbl)
{
    constexpr int W = 4;
    hipStream_t st = (hipStream_t)stream; const uint32_t n_max = p.n_max;
    const bool beside = !sw.no_overlap && aux_ready();
    hipStream_t xs = beside ? (hipStream_t)aux_stream : st;
    if (beside) { HIP_TRY(hipEventRecord((hipEvent_t)ev_fork, st)); HIP_TRY(hipStreamWaitEvent(xs, (hipEvent_t)ev_fork, 0)); }
    tick(5, false, xs);
    if (n_max < XXH_LANE4_BELOW)
        hipLaunchKernelGGL((k_xxh32_blocks4<1>), dim3(n_max), dim3(64), beside ? (12u << 10) : XXH_SPREAD_LDS, xs, (uint8_t*)j.d_frame, tbl, res, n_max, 1u, (FinishVerdict*)bad.p);
    else
        hipLaunchKernelGGL((k_xxh32_blocks<W>), dim3((n_max + W - 1) / W), dim3(64 * W), 0, xs, (uint8_t*)j.d_frame, tbl, res, n_max, 1u, (FinishVerdict*)bad.p);
    tick(5, true, xs);
    if (beside) { HIP_TRY(hipEventRecord((hipEvent_t)ev_join, xs)); aux_pending = true; }
    return 0;
}

// Stage 3: the sequence index - the one that came with the call, or one made here.  ix->d stays null when the indexed kernels do not run.
size_t lz4f_mi355x_engine::dec_index(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut* tbl, IndexSrc* ix, uint32_t* path)
{
    if (p.mode != 'f' || sw.no_index) return 0;
    hipStream_t st = (hipStream_t)stream;
    IndexSrc x{p.ix_by_trailer ? IndexSrc::TRAILER : IndexSrc::GIVEN, j.d_index, j.index_size, j.ix_seqs, j.ix_entries};
    // How many sequences and entries the index holds comes with THIS call (the trailer's footer, the self-index scan, or one
    // read of the index header for the explicit-index entry point): it sizes the descriptor workspace and decides whether a
    // dense frame's scratch is worth having.  Nothing is carried over from earlier calls; the device checks the real header
    // against the workspace (k_check_index) and hands the call to the generic decoder if it does not fit.
    // A linked frame is one match chain without a usable index (seconds instead of milliseconds on dense data), so for
    // those a header that is not the index's drops it (a host synchronisation, ~30 us): the compressor marks an index
    // unusable when the stream had more sequences than it had room for, and then one is made here instead.
    if (j.d_index && j.index_size >= sizeof(IxHeader) && !p.ix_by_trailer && (j.linked || !j.ix_seqs)) {
        IxHeader hd; memset(&hd, 0, sizeof(hd));
        HIP_TRY(hipMemcpyAsync(&hd, j.d_index, sizeof(hd), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hd.magic == IX_MAGIC && hd.stride == IX_STRIDE) { x.seqs = hd.total_seqs; x.entries = hd.total_entries; x.from = IndexSrc::HEADER; }
        else if (j.linked) x = IndexSrc();
    }
    if (!x.d && p.self_index)
        if (size_t e = dec_self_index(j, p, res, tbl, !j.linked, &x)) return e;
    const bool self = x.from == IndexSrc::SELF_LINKED || x.from == IndexSrc::SPX;
    if (self) *path |= LZ4F_MI355X_PATH_SELF_INDEX;
    // (linked frames: only with a table that has every block's output position - the compressor's, or the one just made)
    if (!x.d || x.size < sizeof(IxHeader) || (j.linked && !self && !((p.given || p.ix_by_trailer) && j.hist0 <= 65536))) return 0;
    if ((uint64_t)x.seqs > (uint64_t)x.entries * (IX_STRIDE + 1) || x.entries > (x.size - sizeof(IxHeader)) / sizeof(IxEntry)) x.seqs = 0;      // (not a count this index can hold)
    *ix = x;
    return 0;
}

// A frame without an index (a foreign one: the reference's default output, `lz4 -c`, LZ4F_compressFrame): the index is made here, and the same
// kernels as with the compressor's index take the frame.  A linked frame's: a lane per block walks the payload (parsing needs no history).  Big
// independent blocks' (spx_walk): lanes that start at guessed tokens cut the blocks into stretches, stitched where they meet (decode_spx.cuh).
// A scan places the blocks; its totals, read back (a host synchronisation), size the index.  Dense payloads (k_density_probe) and anything
// odd leave the frame to the generic decoders.
// the stretch points' workspace (decode_spx.cuh): SPX_MAXPT + 1 points per block, then a count per block.  Returns where the counts are.
static size_t spx_carve(Carve& c, uint32_t n_max)
{
    c.take((size_t)n_max * (SPX_MAXPT + 1) * sizeof(SpxPoint));
    return c.take((size_t)n_max * 4 + 64);
}
size_t lz4f_mi355x_engine::dec_self_index(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut* tbl, bool spx_walk, IndexSrc* ix)
{
    hipStream_t st = (hipStream_t)stream; const uint32_t n_max = p.n_max, cpb = j.block_size / pick_chunk_size(j.block_size);
    const size_t fixed = ix_entries_at(n_max, cpb);
    Carve sp{spx}; const size_t spx_cnt_at = spx_carve(sp, n_max);
    if (selfcnt.ensure((size_t)n_max * 8 + 64) || seqcnt.ensure(ixctl_bytes(n_max)) || selfix.ensure(fixed + 64) || density.ensure(64) || (spx_walk && sp.ensure()))
        return make_err(LZ4F_ERROR_allocation_failed);
    uint32_t* cnt = (uint32_t*)selfcnt.p; uint32_t* osz = cnt + n_max;
    IxCtl* ctl = (IxCtl*)seqcnt.p; Density* dens = (Density*)density.p;
    HIP_TRY(hipMemsetAsync(ctl, 0, spx_walk ? sizeof(IxCtl) : offsetof(IxCtl, window), st));      // (the walkers and the scan use the words in front of `window`; SPX_PROF counts further back)
    hipLaunchKernelGGL(k_density_probe, dim3(1), dim3(64), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl, res, n_max, dens);
    if (spx_walk)
        hipLaunchKernelGGL(k_spx_index, dim3(n_max), dim3(SPX_MAXSEG), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl, res, n_max, cnt, osz,
                           sp.at<SpxPoint>(0), sp.at<uint32_t>(spx_cnt_at), ctl, sw.no_density_probe ? (const uint32_t*)nullptr : (const uint32_t*)&dens->not_dense);
    else {
        hipLaunchKernelGGL((k_selfindex_walk_wave<0, 4>), dim3((n_max + 3) / 4), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl,
                           res, n_max, cnt, osz, (void*)nullptr, ctl, (const uint32_t*)&dens->dense);
        hipLaunchKernelGGL(k_selfindex_walk<0>, dim3((n_max + 255) / 256), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl,
                           res, n_max, cnt, osz, (void*)nullptr, ctl, (const uint32_t*)&dens->not_dense);
    }
    IxCtl tot;                                                           // (the scan's verdict and totals: the words in front of chain_total are read back)
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(k_selfindex_scan, dim3(1), dim3(1024), 0, st, tbl, res, n_max, (const uint32_t*)cnt, (const uint32_t*)osz,
                           selfix.p, cpb, (uint64_t)j.dst_cap, j.block_size, ctl, spx_walk ? 1u : 0u);
        if (pass == 1) break;
        HIP_TRY(hipMemcpyAsync(&tot, ctl, offsetof(IxCtl, chain_total), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (spx_walk && sw.prof) fprintf(stderr, "spx: flags %u, %u sequences in %u blocks, %u stretches walked by the stitching thread\n", tot.gave_up, tot.n_seqs, n_max, tot.spx_stitched);
#ifdef SPX_PROF
        SpxProf y;
        if (spx_walk && hipMemcpy(&y, &ctl->spx_prof, sizeof(y), hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "spx lanes: hit the hop cap %u, without a start %u, started at their segment's first byte %u, ran into something %u; most sequences in one lane %u\n", y.hop_cap, y.no_start, y.at_seg_start, y.ran_into, y.most_seqs);
            fprintf(stderr, "spx cycles: guess max %u avg %u, walk max %u avg %u, stitch max %u avg %u, workgroup max %u (waves %u)\n", y.guess_max, (unsigned)(((unsigned long long)y.guess_sum << 8) / (2 * n_max)), y.walk_max, (unsigned)(((unsigned long long)y.walk_sum << 8) / (2 * n_max)), y.stitch_max, (unsigned)(((unsigned long long)y.stitch_sum << 8) / n_max), y.wg_max, 2 * n_max);
        }
#endif
        if (tot.gave_up != 0 || tot.n_seqs == 0) break;
        const void* before = selfix.p;
        if (selfix.ensure(fixed + (size_t)tot.n_entries * sizeof(IxEntry) + 64)) return make_err(LZ4F_ERROR_allocation_failed);
        if (selfix.p == before) break;                                   // (same buffer: the block table is already in it)
    }
    if (tot.gave_up != 0 || tot.n_seqs == 0) return 0;
    if (!spx_walk) {                                                     // (the linked frame's walkers again, filling the index in)
        hipLaunchKernelGGL((k_selfindex_walk_wave<1, 4>), dim3((n_max + 3) / 4), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl,
                           res, n_max, cnt, osz, selfix.p, ctl, (const uint32_t*)&dens->dense);
        hipLaunchKernelGGL(k_selfindex_walk<1>, dim3((n_max + 255) / 256), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl,
                           res, n_max, cnt, osz, selfix.p, ctl, (const uint32_t*)&dens->not_dense);
    }
    *ix = IndexSrc{spx_walk ? IndexSrc::SPX : IndexSrc::SELF_LINKED, selfix.p, fixed + (size_t)tot.n_entries * sizeof(IxEntry), tot.n_seqs, tot.n_entries};
    return 0;
}

// Stage 4: the indexed decode.  Descriptors from the sequence index: a lane per entry parses, a lane per sequence resolves direct
// matches, a workgroup per block copies - or, for independent blocks that are not dense, one kernel does all three.
// *ix_flags: the indexed kernels' "gave up" word, when they were launched.
size_t lz4f_mi355x_engine::dec_indexed(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut* tbl, const IndexSrc& ix, const uint32_t** ix_flags, uint32_t* path)
{
    if (!ix.d) return 0;
    hipStream_t st = (hipStream_t)stream; void* d_index = ix.d;
    const uint32_t chunk = pick_chunk_size(j.block_size), cpb = j.block_size / chunk, n_ix = p.n_ix;
    if ((size_t)ix.seqs + 4096 > ix_seq_cap) ix_seq_cap = (size_t)ix.seqs + ix.seqs / 4 + 4096;
    if (!ix.seqs) return 0;
    Carve dc{desc}; dc.take((ix_seq_cap + 64) * sizeof(SeqDesc));              // the descriptors, then a resolved source per descriptor
    const size_t dsrc_at = dc.take((ix_seq_cap + 64) * 4);
    if (dc.ensure() || seqcnt.ensure(ixctl_bytes(p.n_max))) return make_err(LZ4F_ERROR_allocation_failed);
    IxCtl* ctl = (IxCtl*)seqcnt.p;
    HIP_TRY(hipMemsetAsync(ctl, 0, j.linked ? ixctl_cleared(p.n_max) : sizeof(IxCtl), st));      // the control block (+ per block of a linked frame: the "done" word and the count of published ranges)
    Carve sp{spx}; const size_t spx_cnt_at = spx_carve(sp, p.n_max);              // (dec_self_index filled it, if the index is its stretches)
    unsigned long long* iprof = (unsigned long long*)(sw.prof ? prof_buf() : nullptr);
    tick(8, false);
    hipLaunchKernelGGL(k_check_index, dim3(1), dim3(64), 0, st, (const void*)d_index, (uint64_t)ix.size, n_ix, cpb, chunk,
                       (uint64_t)ix_seq_cap, ctl, (const ResultRec*)res);
    // the whole block table, before any kernel behind writes (the index is input)
    hipLaunchKernelGGL(k_check_blocks, dim3((n_ix + 255) / 256), dim3(256), 0, st, (const void*)d_index, (const BlockOut*)tbl, (const ResultRec*)res, n_ix,
                       ctl);
    const IxRoute r = ix_route(j, sw, n_ix, ix.seqs);
    *ix_flags = &ctl->gave_up;
    *path |= LZ4F_MI355X_PATH_INDEXED;
    if (r.selffed) {
        tick(8, true); tick(9, false);
        // k_copy_selffed in the workgroup shape of the block size, with the block's runs from the index or from the stitched stretches
        auto selffed = [&](auto src) {
            using S = decltype(src);
            if (j.block_size <= (1u << 20))
                hipLaunchKernelGGL((k_copy_selffed<FzCfgS4, S>), dim3(n_ix), dim3(64 * 4), 0, st, j.d_frame, (uint64_t)j.frame_cap, j.d_dst, tbl, (const ResultRec*)res, n_ix,
                                   (const void*)d_index, (SeqDesc*)desc.p, ctl, iprof, src, sw.feed_round, j.block_size);
            else
                hipLaunchKernelGGL((k_copy_selffed<FzCfgS8, S>), dim3(n_ix), dim3(64 * 8), 0, st, j.d_frame, (uint64_t)j.frame_cap, j.d_dst, tbl, (const ResultRec*)res, n_ix,
                                   (const void*)d_index, (SeqDesc*)desc.p, ctl, iprof, src, sw.feed_round, j.block_size);
        };
        if (ix.from == IndexSrc::SPX) selffed(FzSrcSpx{sp.at<const SpxPoint>(0), sp.at<const uint32_t>(spx_cnt_at)});
        else selffed(FzSrcIx{(const void*)d_index, n_ix});
        tick(9, true);
        return 0;
    }
    // the chain: parse, resolve direct matches, trace dense frames, copy, check the tails
    uint32_t* done = ixctl_done(ctl);
    const uint32_t lk = j.linked ? 1u | (uint32_t)sw.chain_gate << 1 : 0u;      // (bits 1..: chain gate, see k_copy_indexed)
    const uint32_t n_lanes = ix.entries > n_ix ? ix.entries : n_ix;     // (grid-stride inside: a hint is enough)
    if (ix.from == IndexSrc::SPX)                                                 // (no entries: the stretches between the blocks' check lines)
        hipLaunchKernelGGL(k_spx_parse, dim3(n_ix), dim3(128), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl, (const ResultRec*)res, n_ix,
                           d_index, sp.at<const SpxPoint>(0), sp.at<const uint32_t>(spx_cnt_at), (SeqDesc*)desc.p, ctl);
    else
        hipLaunchKernelGGL(k_parse_indexed, dim3((n_lanes + 255) / 256), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap,
                           (const BlockOut*)tbl, d_index, n_ix, (SeqDesc*)desc.p, ctl, lk, (uint64_t)j.hist0);
    const uint64_t trace_span = (uint64_t)n_ix * j.block_size;            // (the last block may be short)
    const uint32_t res_gy = j.block_size >= (1u << 19) ? j.block_size >> 18 : 1u;
    uint32_t gate = r.gate;
    Carve pt{postab}; pt.take((size_t)(trace_span >> 6) * 4);          // a word per 64 output bytes, then the regions' byte counts
    const size_t region_at = pt.take(((size_t)(trace_span >> IXT_REGION_LOG) + 4) * 4 + 512, 256);
    if (gate && pt.ensure()) gate = 0;                              // (no memory for the position table: the copiers do it)
    if (gate && r.doubling)                                        // (dense by the sequence density: no need to resolve anything)
        hipLaunchKernelGGL(k_dense_gate, dim3(1), dim3(64), 0, st, ctl, gate, (const BlockOut*)tbl, (const ResultRec*)res, n_ix, 1u, 1u);
    uint32_t* dsrc = sw.no_resolve ? nullptr : dc.at<uint32_t>(dsrc_at);
    if (dsrc)
        hipLaunchKernelGGL(k_resolve_direct, dim3(n_ix, res_gy), dim3(256), 0, st, d_index, (const BlockOut*)tbl, (const ResultRec*)res, n_ix, (const SeqDesc*)desc.p,
                           dsrc, ctl, (iprof ? 1u : 0u) | (gate ? 2u : 0u), lk);
    if (iprof) {                                                   // developer aid: how many matches are direct
        IxCtl c;
        if (prof_read(st, &c, ctl, sizeof(c))) {
            fprintf(stderr, "indexed: flags %u, matches direct after parse %u, resolved %u, left to the chain %u\n", c.gave_up, c.m_direct, c.m_resolved, c.m_chain);
            fprintf(stderr, "indexed (linked): %u matches stay on the chain, %u of them reach into the block in front (%u blocks); not resolved because: beyond one block %u, source straddles two runs %u, run-length source %u, hop limit %u\n", c.chain_total, c.m_reach_front, n_ix, c.why_far, c.why_straddle, c.why_runlen, c.why_hops);
        }
    }
    // dense frames (text): no chain at all, every output byte traced to its literal (see k_trace_copy)
    hipLaunchKernelGGL(k_dense_gate, dim3(1), dim3(64), 0, st, ctl, gate, (const BlockOut*)tbl, (const ResultRec*)res, n_ix, 0u, res_gy);
    if (gate) {
        hipLaunchKernelGGL(k_build_postab, dim3(n_ix, res_gy), dim3(256), 0, st, d_index, (const BlockOut*)tbl, (const ResultRec*)res, n_ix,
                           (const SeqDesc*)desc.p, (uint32_t*)postab.p, ctl);
        const uint64_t n_thr = (trace_span + IXT_TB - 1) / IXT_TB;
        // if the last index seen here was of a dense stream (the device decides about THIS one, but the
        // scratch - 4 bytes per output byte - and 18 launches are the host's to spend): one hop per byte, then pointer doubling
        const uint32_t pd_grid = (uint32_t)((trace_span / 4 + 255) / 256), pd_ngrp = pd_grid * 4u;      // (k_pd_round: a wave per 256 bytes)
        Carve pd{pdbuf}; pd.take((size_t)trace_span * 4);              // a word per output byte, the bytes still open after each round, a byte pair per group
        const size_t remaining_at = pd.take((IXP_ROUNDS + 1) * IXP_STRIPES * 4, 256), pd_grp_at = pd.take(2 * (size_t)pd_ngrp + 256, 256);
        if (r.doubling && !pd.ensure()) {
            *path |= LZ4F_MI355X_PATH_DOUBLING;
            uint32_t* remaining = pd.at<uint32_t>(remaining_at);
            if (hipMemsetAsync(remaining, 0, (IXP_ROUNDS + 1) * IXP_STRIPES * 4, st) != hipSuccess) return make_err(LZ4F_ERROR_GENERIC);
            hipLaunchKernelGGL(k_pd_init, dim3((uint32_t)((n_thr + 255) / 256)), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap, j.d_dst, (const BlockOut*)tbl,
                               (const ResultRec*)res, n_ix, d_index, (const SeqDesc*)desc.p, (const uint32_t*)dsrc, (const uint32_t*)postab.p, ctl,
                               lk & 1u, (uint32_t)j.block_size, (uint64_t)j.hist0, (uint32_t*)pdbuf.p, remaining);
            for (uint32_t rd = 1; rd <= IXP_ROUNDS; rd++)
                hipLaunchKernelGGL(k_pd_round, dim3(pd_grid), dim3(256), 0, st, j.d_dst, (uint32_t*)pdbuf.p, (const BlockOut*)tbl,
                                   (const ResultRec*)res, n_ix, rd, remaining, ctl, pd.at<uint8_t>(pd_grp_at), pd_ngrp);
            hipLaunchKernelGGL(k_pd_verdict, dim3(1), dim3(64), 0, st, ctl, (const uint32_t*)remaining);
            if (iprof) { static uint32_t t[(IXP_ROUNDS + 1) * IXP_STRIPES]; if (prof_read(st, t, remaining, sizeof(t))) { fprintf(stderr, "doubling: bytes open after each round:"); for (uint32_t rd = 0; rd <= IXP_ROUNDS; rd++) { uint64_t sum = 0; for (uint32_t q = 0; q < IXP_STRIPES; q++) sum += t[rd * IXP_STRIPES + q]; fprintf(stderr, " %llu", (unsigned long long)sum); } fprintf(stderr, "\n"); } }
        } else {
            *path |= LZ4F_MI355X_PATH_TRACE_HOPS;
            uint32_t* region_cnt = pt.at<uint32_t>(region_at);
            if (hipMemsetAsync(region_cnt, 0, ((size_t)(trace_span >> IXT_REGION_LOG) + 2) * 4, st) != hipSuccess) return make_err(LZ4F_ERROR_GENERIC);
            const uint32_t tc_wg = (uint32_t)((n_thr + 255) / 256);
            hipLaunchKernelGGL(k_trace_copy, dim3(std::min<uint32_t>(tc_wg, 8192u)), dim3(256), 0, st, j.d_frame, (uint64_t)j.frame_cap, j.d_dst, (const BlockOut*)tbl,
                               (const ResultRec*)res, n_ix, d_index, (const SeqDesc*)desc.p, (const uint32_t*)dsrc, (const uint32_t*)postab.p, ctl,
                               lk & 1u, (uint32_t)j.block_size, (uint64_t)j.hist0, region_cnt, iprof ? 1u : 0u, tc_wg);
            IxCtl t;
            if (iprof && prof_read(st, &t, ctl, sizeof(t)) && t.dense) fprintf(stderr, "traced: %llu turns for %u pieces (%u read from the output), deepest thread %u turns\n", t.t_turns, t.t_pieces, t.t_from_out, t.t_deepest);
        }
    }
    tick(8, true); tick(9, false);
    auto copy = [&](auto cfg) {
        using C = decltype(cfg);
        hipLaunchKernelGGL(k_copy_indexed<C>, dim3((n_ix + p.group - 1) / p.group), dim3(64 * C::WAVES), 0, st, j.d_frame, j.d_dst, tbl, (const ResultRec*)res, n_ix,
                           d_index, (const SeqDesc*)desc.p, (const uint32_t*)dsrc, ctl, iprof, lk, done, p.group, (uint64_t)j.hist0, p.wait_ticks);
    };
    if (j.block_size <= (1u << 20)) copy(FzCfg<4>()); else copy(FzCfg<8>());
    tick(9, true);
    IxCtl y;
    if (iprof && j.linked && prof_read(st, &y, ctl, sizeof(y))) fprintf(stderr, "indexed (linked): blocks that found the block in front at state 3: %u (of those, had to wait for all of it: %u); blocks with set-aside matches %u (block in front already done: %u)\n", y.l_state3, y.l_state3_waited, y.l_setaside, y.l_front_done);
    hipLaunchKernelGGL(k_check_tails, dim3((n_ix + 255) / 256), dim3(256), 0, st, tbl, (const ResultRec*)res, n_ix, d_index,
                       (const SeqDesc*)desc.p, (uint64_t)ix_seq_cap, j.block_size, (const IxCtl*)ctl);
    return 0;
}

// Stage 5: the generic decoders.  Each runs only if the one in front gave up: only_if is the indexed kernels' flags word (null: none
// ran), then the window kernel's fallback word, then the density probe's verdict.
size_t lz4f_mi355x_engine::dec_generic(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut* tbl, const uint32_t* only_if, uint32_t* path)
{
    constexpr int W = 4;
    hipStream_t st = (hipStream_t)stream; const uint32_t n_max = p.n_max;
    if (p.mode == 'f') {
        unsigned long long* prof = (unsigned long long*)(sw.prof ? prof_buf() : nullptr);
        const bool indexed = only_if != nullptr;
        if (p.windowed) {
            *path |= LZ4F_MI355X_PATH_WINDOW;
            if (!indexed && seqcnt.ensure(256)) return make_err(LZ4F_ERROR_allocation_failed);
            // (behind the indexed kernels the verdict has its place in their control block; without them the buffer holds nothing else)
            LinkedFallback* fb = indexed ? &((IxCtl*)seqcnt.p)->window : (LinkedFallback*)seqcnt.p;
            hipLaunchKernelGGL(k_decode_linked, dim3(1), dim3(64 * LK_WAVES), 0, st, j.d_frame, j.d_dst, j.dst_cap, tbl,
                               (const ResultRec*)res, n_max, j.block_size, j.hist0, fb, only_if);
            only_if = &fb->gave_up;
            LinkedFallback dbg;                                           // developer aid: why the windowed kernel stopped, if it did
            if (sw.prof && prof_read(st, &dbg, fb, sizeof(dbg))) fprintf(stderr, "k_decode_linked: fallback %u why %u block %u\n", dbg.gave_up, dbg.why, dbg.block);
        }
        *path |= LZ4F_MI355X_PATH_FUSED;
        // big independent blocks and no index to go by: a look at the payload decides between the fused workgroups and - dense data -
        // the wave-per-block decoder (k_density_probe); both are launched, one of them returns at once
        if (!indexed && !j.linked && !sw.no_density_probe) {
            if (density.ensure(64)) return make_err(LZ4F_ERROR_allocation_failed);
            Density* dens = (Density*)density.p;
            hipLaunchKernelGGL(k_density_probe, dim3(1), dim3(64), 0, st, j.d_frame, (uint64_t)j.frame_cap, (const BlockOut*)tbl, (const ResultRec*)res, n_max, dens);
            if (p.relay) {
                *path |= LZ4F_MI355X_PATH_WORKGROUP_PER_BLOCK;
                hipLaunchKernelGGL((k_decode_blocks_relay<RELAY_W, RELAY_S>), dim3(n_max), dim3(64 * (RELAY_W + RELAY_S + 3)), 0, st, j.d_frame, j.d_dst, tbl, (const ResultRec*)res, n_max, (uint64_t)j.frame_cap,
                                   (const uint32_t*)&dens->dense);
            } else
                hipLaunchKernelGGL((k_decode_blocks<W>), dim3((n_max + W - 1) / W), dim3(64 * W), 0, st, j.d_frame, j.d_dst, j.dst_cap, tbl, (const ResultRec*)res,
                                   n_max, 0u, j.block_size, j.hist0, (uint64_t)j.frame_cap, (const uint32_t*)&dens->dense);
            only_if = &dens->not_dense;
            *path |= LZ4F_MI355X_PATH_WAVE_PER_BLOCK;
        }
        auto fused = [&](auto cfg) {                                   // (a linked frame: one workgroup, in the 8-wave shape)
            using C = decltype(cfg);
            hipLaunchKernelGGL(k_decode_blocks_fused<C>, dim3(j.linked ? 1u : n_max), dim3(64 * C::WAVES), 0, st, j.d_frame, j.d_dst, j.dst_cap, tbl,
                               (const ResultRec*)res, n_max, j.linked ? 1u : 0u, j.block_size, j.hist0, prof, only_if);
        };
        if (p.small) fused(FzCfg<4>()); else fused(FzCfg<8>());
    } else {
        *path |= LZ4F_MI355X_PATH_WAVE_PER_BLOCK;
        hipLaunchKernelGGL((k_decode_blocks<W>), dim3(j.linked ? 1u : (n_max + W - 1) / W), dim3(64 * W), sw.dblk_lds, st, j.d_frame, j.d_dst, j.dst_cap, tbl, (const ResultRec*)res,
                           n_max, j.linked ? 1u : 0u, j.block_size, j.hist0, (uint64_t)j.frame_cap);
    }
    return 0;
}

// Stage 6: what every call ends with - the tight last block, the verdicts, the result record and the content checksum.
size_t lz4f_mi355x_engine::dec_finish(const DecompressJob& j, const DecodePlan& p, ResultRec* res, BlockOut* tbl, const uint32_t* ix_flags, uint32_t path)
{
    hipStream_t st = (hipStream_t)stream; const uint32_t n_max = p.n_max;
    tick(7, false);
    // liblz4 judges a block against maxBlockSize whatever room the caller leaves it.  Only a walked frame's last block can be left less
    // (every other block sits below a provisional block's room the walk found inside the buffer), and only when the capacity is not a
    // multiple of the block size: a last block that failed in that room is decoded again with a whole block's room, and copied out if it fits.
    if (n_max && !p.given && j.block_size && j.dst_cap % j.block_size != 0) {
        if (tight.ensure((size_t)65536 + j.block_size + 64)) return make_err(LZ4F_ERROR_allocation_failed);
        hipLaunchKernelGGL(k_redo_tight_block, dim3(1), dim3(64), 0, st, j.d_frame, (uint64_t)j.frame_cap, j.d_dst, (uint64_t)j.dst_cap, tbl,
                           (const ResultRec*)res, n_max, j.linked ? 1u : 0u, j.block_size, (uint64_t)j.hist0, (uint8_t*)tight.p);
    }
    const bool check_here = n_max <= 64;                              // (the finishing wave looks at a few blocks itself: a launch less)
    if (n_max && !check_here) hipLaunchKernelGGL(k_finish_check, dim3((n_max + 255) / 256), dim3(256), 0, st, (const BlockOut*)tbl, (const ResultRec*)res, n_max, j.linked ? 1u : 0u, j.block_size, (FinishVerdict*)bad.p);
    hipLaunchKernelGGL(k_finish_decode, dim3(1), dim3(64), 0, st, j.d_dst, tbl, res, n_max, j.linked ? 1u : 0u, j.block_size,
                       (const FinishVerdict*)bad.p, j.block_checksum ? 1u : 0u, path, ix_flags, check_here ? 1u : 0u, (uint64_t)j.dst_cap);
    if (j.content_checksum && !p.given && !sw.no_content_check)      // (a whole frame was walked: res->consumed is behind its checksum word)
        hipLaunchKernelGGL(k_xxh32_content, dim3(1), dim3(64), 0, st, (const uint8_t*)j.d_dst, 0ull, (uint8_t*)j.d_frame, res, 1u);
    tick(7, true);
    return 0;
}

size_t lz4f_mi355x_engine::launch_decompress(const DecompressJob& j, lz4f_mi355x_result* d_res)
{
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (!d_res) { if (res.ensure(sizeof(ResultRec))) return make_err(LZ4F_ERROR_allocation_failed); d_res = (lz4f_mi355x_result*)res.p; }
    if (bad.ensure(64)) return make_err(LZ4F_ERROR_allocation_failed);
    ResultRec* r = (ResultRec*)d_res;
    const DecodePlan p = decode_plan(j, sw, device_cus(device));
    uint32_t path = 0;                                               // LZ4F_MI355X_PATH_*: reported in result.flags
    for (int i = 4; i < 10; i++) ev_used[i] = false;
    ev_used[11] = false;
    if (aux_pending) { HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)ev_join, 0)); aux_pending = false; }      // (a call that left early: its forked work first)
    // every exit behind the fork joins: an error return (allocation, a HIP call) leaves the main stream waiting for the forked verification, so
    // that whatever the caller enqueues or frees behind a synchronisation of its stream comes after the kernel that still reads the frame
    struct AuxJoin {
        lz4f_mi355x_engine* e; hipStream_t st;
        ~AuxJoin() { if (e->aux_pending && hipStreamWaitEvent(st, (hipEvent_t)e->ev_join, 0) == hipSuccess) e->aux_pending = false; }
    } aux_join{this, st};
    tick(11, false);
    BlockOut* tbl;
    if (size_t e = dec_table(j, p, r, &tbl, &path)) return e;
    const uint32_t* ix_flags = nullptr;                              // the indexed kernels' "gave up" word, if they were launched
    if (p.n_max) {
        if (j.block_checksum) { if (size_t e = dec_checksums(j, p, r, tbl)) return e; }
        tick(6, false);
        IndexSrc ix;
        if (size_t e = dec_index(j, p, r, tbl, &ix, &path)) return e;
        if (size_t e = dec_indexed(j, p, r, tbl, ix, &ix_flags, &path)) return e;
        if (size_t e = dec_generic(j, p, r, tbl, ix_flags, &path)) return e;
        tick(6, true);
    }
    if (aux_pending) { HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)ev_join, 0)); aux_pending = false; }
    if (size_t e = dec_finish(j, p, r, tbl, ix_flags, path)) return e;
    tick(11, true);
    HIP_TRY(hipGetLastError());
    return 0;
}


// ------------------------------------------------------------------------------------------------
// C ABI: engine + device-pointer entry points
// ---- the batch calls: many frames, one call, no host read ----
constexpr uint32_t BATCH_GRID = 8192;       // workgroups at most of a kernel that strides over a table's entries in use
constexpr uint32_t PK_GRID = 65536;         // the same of the pack's copy kernel: a workgroup per tile up to 1 GiB of output (the dispatcher deals them as CUs come free), striding beyond

// what every batch call begins with, once its own argument checks are through: its pointers, the device, and the work an earlier
// call left on the aux stream (aux_pending is set here only after launch_decompress's error path failed to join it)
static size_t batch_begin(lz4f_mi355x_engine* e, const char* call, bool pointers_ok)
{
    if (!pointers_ok) { set_last_error("%s: null pointer", call); return make_err(LZ4F_ERROR_GENERIC); }
    if (hipSetDevice(e->device) != hipSuccess) { set_last_error("hipSetDevice failed"); return make_err(LZ4F_ERROR_GENERIC); }
    if (e->aux_pending) { HIP_TRY(hipStreamWaitEvent((hipStream_t)e->stream, (hipEvent_t)e->ev_join, 0)); e->aux_pending = false; }
    return 0;
}
static size_t batch_end(const char* call)
{
    if (hipGetLastError() != hipSuccess) { set_last_error("%s: launch failed", call); return make_err(LZ4F_ERROR_GENERIC); }
    return 0;
}
// How a batch entry point opens.  -> true: the call ends here and returns r - no engine, or no frames and nothing to do (batch_idle);
// its pointers, the device, the aux stream (batch_open).  The set calls judge their set between the two; the compress calls judge
// their preferences and the level in front of `n == 0` and open for themselves (compress_frames)
static bool batch_idle(const lz4f_mi355x_engine* e, uint32_t n, size_t& r)
{
    r = e ? 0 : make_err(LZ4F_ERROR_GENERIC);
    return !e || n == 0;
}
static bool batch_open(lz4f_mi355x_engine* e, uint32_t n, const char* call, bool pointers_ok, size_t& r)
{
    return batch_idle(e, n, r) || (r = batch_begin(e, call, pointers_ok)) != 0;
}
// a table's entries, from the call's arguments alone (a slice's place is a 32-bit entry number)
static uint64_t batch_table_cap(uint32_t n_frames, uint64_t shared)
{
    return std::min<uint64_t>((uint64_t)n_frames + shared + 1, 0xFFFFFFF0ull);
}
// the grid of a kernel that strides over up to `items` table entries, `per_wg` to a workgroup at a time
static dim3 batch_grid(uint64_t items, uint32_t per_wg, uint32_t most = BATCH_GRID)
{
    return dim3((uint32_t)std::min<uint64_t>((items + per_wg - 1) / per_wg, most));
}
// what the decode and compress entry points pass along unchanged: the frames' spans in d_src and their windows in d_dst
struct BatchSpans {
    uint32_t n_frames;
    const void* d_src; size_t srcBytes; const uint64_t* d_src_off;
    void* d_dst; size_t dstBytes; const uint64_t* d_dst_off;
};

// A prepared dictionary (lz4f_mi355x_dev_createCDict / _createCDictHC): its engine's, never written after the stream has run its creation.
// One device allocation: the digest (SOLO_DIGEST_BYTES: the finder's table and tags, seeded), the hash-chain finder's digest where asked
// for (lz4f_mi355x_dev_createCDictHC: hc_digest_bytes(len), head and chain), then the dictionary's last `len` (<= 64 KiB) bytes
struct lz4f_mi355x_cdict {
    lz4f_mi355x_engine* engine = nullptr;
    EncDict dict;                          // the owned copy's tail and its digests (hc_digest NULL: made by createCDict); len 0: an empty dictionary
    bool hc = false;                       // made by createCDictHC: serves levels 3-12 too
    void* mem = nullptr;                   // the allocation; NULL: an empty dictionary
};

// A set of prepared dictionaries (lz4f_mi355x_dev_createDictSet, dictset.cuh): its engine's; the members are borrowed.  One device
// allocation, uploaded on the engine's stream at creation and never written again: DsMember[count], the IDs sorted, the members in
// that order
struct lz4f_mi355x_dictset {
    lz4f_mi355x_engine* engine = nullptr;
    DsView view;                           // the device table (count 0: nothing allocated)
    bool all_hc = true;                    // every non-empty member was made by createCDictHC: the set serves levels 3-12
    void* mem = nullptr;
    std::vector<uint8_t> staged;           // the table as it was uploaded (kept: the copy may read it after createDictSet returned)
};

// A batch call's dictionary in one value: none (BatchDict{}), one for every frame, or a set with the frames' slots
struct BatchDict {
    EncDict one;                           // a raw dictionary's tail (the decoders take just that, DictTail), or a prepared one's with its digests
    bool hc_ok = false;                    // `one` was made for levels 3-12 (it may still lack one.hc_digest: 1-3 bytes, which the finder ignores)
    const lz4f_mi355x_dictset* set = nullptr;      // frame i with the member d_slot[i] names, or (the decoder, d_slot NULL) its header
    const uint32_t* d_slot = nullptr;
    bool any() const { return set || one.len; }                       // (which members the frames name is known on the device only)
    bool serves_hc() const { return set ? set->all_hc : hc_ok; }      // levels 3-12: only with the hash-chain digest, every member of a set
};

// The finder kernel of a batch (encode_batch.cuh) and the most workgroups it gets: by the level, and by what the dictionary brings
template <typename D> struct BcFind { BcFinder<D> kernel; uint32_t most_wgs, threads; };
static BcFind<EncDict> bc_finder(bool hc, const EncDict& dc)
{
    // (levels 3-12 without the digest: no dictionary, or a prepared one of 1-3 bytes, which the finder ignores)
    if (hc) return {dc.len && dc.hc_digest ? k_bc_find_hc<true> : k_bc_find_hc<false>, BATCH_GRID / 4, 64 * HC_WAVES};
    return {!dc.len ? k_bc_find_solo<false, false> : dc.solo_digest ? k_bc_find_solo<true, true> : k_bc_find_solo<true, false>, BATCH_GRID * 2, 64};
}
// (a set: the prepared-dictionary finders with each chunk's frame's member, the same grids)
static BcFind<DsView> bc_finder(bool hc, const DsView&)
{
    if (hc) return {k_bc_find_hc<true, DsView>, BATCH_GRID / 4, 64 * HC_WAVES};
    return {k_bc_find_solo<true, true, DsView>, BATCH_GRID * 2, 64};
}

extern "C" {

const char* lz4f_mi355x_last_error(void) { return lz4f::last_error(); }

int lz4f_mi355x_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t lz4f_mi355x_set_device(int device)
{
    int n = lz4f_mi355x_device_count();
    if (device < 0 || device >= n) { set_last_error("device %d out of range (%d devices)", device, n); return make_err(LZ4F_ERROR_GENERIC); }
    lz4f::t_device = device;
    return 0;
}

size_t lz4f_mi355x_engine_create(lz4f_mi355x_engine** out, int device, void* hipStream, int borrowStream)
{
    if (!out) return make_err(LZ4F_ERROR_GENERIC);
    return new_engine(out, device, hipStream, borrowStream != 0);
}
size_t lz4f_mi355x_engine_free(lz4f_mi355x_engine* e) { delete e; return 0; }
void lz4f_mi355x_release_engines(void) { lz4f::release_idle_engines(); }
void* lz4f_mi355x_host_alloc(size_t size)
{
    void* p = nullptr;
    if (hipSetDevice(lz4f::selected_device()) != hipSuccess || hipHostMalloc(&p, size ? size : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); set_last_error("hipHostMalloc(%zu) failed", size); return nullptr; }
    return p;
}
void lz4f_mi355x_host_free(void* p) { if (p) (void)hipHostFree(p); }
void* lz4f_mi355x_engine_stream(lz4f_mi355x_engine* e) { return e ? e->stream : nullptr; }

size_t lz4f_mi355x_engine_set_deterministic(lz4f_mi355x_engine* e, int enable)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    if (enable) e->sw.e1_solo |= 1u; else e->sw.e1_solo &= ~1u;
    return 0;
}
size_t lz4f_mi355x_engine_set_timing(lz4f_mi355x_engine* e, int enable)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    e->timing = enable != 0;
    return 0;
}
size_t lz4f_mi355x_engine_get_timing(lz4f_mi355x_engine* e, float* ms) { return lz4f_mi355x_engine_get_timing_n(e, ms, LZ4F_MI355X_TIMING_SLOTS_V1); }
size_t lz4f_mi355x_engine_get_timing_n(lz4f_mi355x_engine* e, float* ms, size_t n)
{
    if (!e || !ms) return make_err(LZ4F_ERROR_GENERIC);
    size_t r = e->sync();
    if (is_err(r)) return r;
    for (int s = 0; s < LZ4F_MI355X_TIMING_SLOTS && (size_t)s < n; s++) {
        ms[s] = 0.f;
        if (e->ev_used[s] && e->ev[2 * s] && e->ev[2 * s + 1]) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, (hipEvent_t)e->ev[2 * s], (hipEvent_t)e->ev[2 * s + 1]) == hipSuccess) ms[s] = t;
        }
    }
    return 0;
}

size_t lz4f_mi355x_dev_workspace_size(size_t srcSize, const LZ4F_preferences_t* prefs)
{
    const size_t bs = block_size_of(prefs ? prefs->frameInfo.blockSizeID : 0);
    if (!bs) return make_err(LZ4F_ERROR_maxBlockSize_invalid);
    const EncShape s = enc_shape(srcSize, (uint32_t)bs);
    const size_t nchunks = s.n_blocks * s.chunks_per_block + 1;
    // (the record pool as an engine with default switches sizes it: 12288 records of 8 bytes per 64 KiB tile = 1.5 bytes per input byte)
    return nchunks * sizeof(ChunkInfo) + (size_t)(rec_pool_at((uint32_t)nchunks) + rec_pool_records((uint32_t)nchunks, s.chunk / 4 + 1, 0)) * 8
           + (s.n_blocks + 1) * (sizeof(BlockOut) + 4) + 4096;
}

// (the index and trailer bounds take an invalid block size ID as 64 KiB)
static EncShape sizing_shape(size_t srcSize, const LZ4F_preferences_t* prefs)
{
    const size_t bs = block_size_of(prefs ? prefs->frameInfo.blockSizeID : 0);
    return enc_shape(srcSize, bs ? (uint32_t)bs : 65536u);
}
size_t lz4f_mi355x_dev_index_size(size_t srcSize, const LZ4F_preferences_t* prefs) { return index_capacity(srcSize, sizing_shape(srcSize, prefs)); }


size_t lz4f_mi355x_trailer_bound(size_t srcSize, const LZ4F_preferences_t* prefs)
{
    return lz4f_mi355x_dev_index_size(srcSize, prefs) + (sizing_shape(srcSize, prefs).n_blocks + 2) * 8 + 128;
}

// A compress call's preferences resolved: p, the caller's copy (NULL: all defaults) with 64 KiB blocks where it names no size, and bs,
// its block size -> 0, or ERROR_maxBlockSize_invalid
static size_t resolve_prefs(const LZ4F_preferences_t* prefs, LZ4F_preferences_t& p, size_t& bs)
{
    memset(&p, 0, sizeof(p));
    if (prefs) p = *prefs;
    if (p.frameInfo.blockSizeID == 0) p.frameInfo.blockSizeID = LZ4F_max64KB;
    bs = block_size_of(p.frameInfo.blockSizeID);
    return bs ? 0 : make_err(LZ4F_ERROR_maxBlockSize_invalid);
}

// the preferences resolved and checked, then the whole-frame job (index_cap: LZ4F_MI355X_INBAND, a given index's capacity, or 0 for none)
static size_t compress_frame(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, const LZ4F_preferences_t* prefs,
                             lz4f_mi355x_result* d_result, lz4f_mi355x_block* d_table, void* d_index, size_t index_cap)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    LZ4F_preferences_t p; size_t bs;
    if (const size_t r = resolve_prefs(prefs, p, bs)) return r;
    if (p.frameInfo.contentSize && p.frameInfo.contentSize != srcSize) return make_err(LZ4F_ERROR_frameSize_wrong);
    const auto j = lz4f_mi355x_engine::make_compress_job((const uint8_t*)d_src, srcSize, 0, (uint32_t)bs, p.frameInfo.blockMode == LZ4F_blockLinked,
                                                         p.frameInfo.blockChecksumFlag != 0, p.compressionLevel, &p);
    return e->launch_compress(j, (uint8_t*)d_dst, dstCapacity, d_result, d_table, d_index, index_cap);
}

size_t lz4f_mi355x_dev_compressFrame(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize,
                                     const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_result, lz4f_mi355x_block* d_table)
{
    return compress_frame(e, d_dst, dstCapacity, d_src, srcSize, prefs, d_result, d_table, nullptr, 0);
}

size_t lz4f_mi355x_dev_compressFrameIndexed(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize,
                                            const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_result, lz4f_mi355x_block* d_table, void* d_index,
                                            size_t indexCapacity)
{
    const bool inband = d_index == nullptr && indexCapacity == LZ4F_MI355X_INBAND;
    if (!e || (!inband && (!d_table || !d_result))) return make_err(LZ4F_ERROR_GENERIC);
    return compress_frame(e, d_dst, dstCapacity, d_src, srcSize, prefs, d_result, d_table, d_index, inband ? LZ4F_MI355X_INBAND : (d_index ? indexCapacity : 0));
}

size_t lz4f_mi355x_dev_decompressBlocksIndexed(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_frame, size_t frameCapacity,
                                               const lz4f_mi355x_block* d_table, uint32_t n_blocks, const LZ4F_frameInfo_t* info,
                                               const void* d_index, size_t indexSize, lz4f_mi355x_result* d_result)
{
    if (!e || !d_table || !info) return make_err(LZ4F_ERROR_GENERIC);
    const size_t bs = block_size_of(info->blockSizeID);
    if (!bs) return make_err(LZ4F_ERROR_maxBlockSize_invalid);
    lz4f_mi355x_engine::DecompressJob j; memset(&j, 0, sizeof(j));
    j.d_frame = (const uint8_t*)d_frame; j.frame_cap = frameCapacity; j.d_dst = (uint8_t*)d_dst; j.dst_cap = dstCapacity; j.hist0 = 0;
    j.block_size = (uint32_t)bs; j.linked = info->blockMode == LZ4F_blockLinked; j.block_checksum = info->blockChecksumFlag != 0;
    j.d_table = d_table; j.n_blocks = n_blocks; j.max_blocks = n_blocks; j.d_index = (void*)d_index; j.index_size = d_index ? indexSize : 0;
    return e->launch_decompress(j, d_result);
}

size_t lz4f_mi355x_dev_decompressFrame(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_frame, size_t frameCapacity,
                                       lz4f_mi355x_result* d_result)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    if (hipSetDevice(e->device) != hipSuccess) { set_last_error("hipSetDevice failed"); return make_err(LZ4F_ERROR_GENERIC); }
    // the descriptor (7..19 bytes) decides block size / linked / checksum flags: peek it (the only host sync here)
    uint8_t hdr[32]; memset(hdr, 0, sizeof(hdr));
    const size_t peek = frameCapacity < 19 ? frameCapacity : 19;
    if (peek < 7) return make_err(LZ4F_ERROR_frameHeader_incomplete);
    TrailerFoot foot; memset(&foot, 0, sizeof(foot));              // the stream's last 32 bytes: this library's trailer, if it is one
    const bool may_trail = frameCapacity >= 64 && ((uintptr_t)d_frame & 15) == 0 && !e->sw.no_trailer;
    if (hipMemcpyAsync(hdr, d_frame, peek, hipMemcpyDeviceToHost, (hipStream_t)e->stream) != hipSuccess ||
        (may_trail && hipMemcpyAsync(&foot, (const uint8_t*)d_frame + frameCapacity - sizeof(foot), sizeof(foot), hipMemcpyDeviceToHost, (hipStream_t)e->stream) != hipSuccess) ||
        hipStreamSynchronize((hipStream_t)e->stream) != hipSuccess) { set_last_error("header peek failed"); return make_err(LZ4F_ERROR_GENERIC); }
    lz4f_mi355x_engine::DecompressJob j; memset(&j, 0, sizeof(j));
    j.d_frame = (const uint8_t*)d_frame; j.frame_cap = frameCapacity; j.d_dst = (uint8_t*)d_dst; j.dst_cap = dstCapacity; j.hist0 = 0;
    j.block_size = 65536; j.linked = false; j.block_checksum = false; j.max_blocks = 1;
    if (rd32le(hdr) == FRAME_MAGIC) {
        ParsedHeader ph;
        size_t hs = parse_frame_header(hdr, peek, &ph);
        if (is_err(hs)) return hs;
        j.block_size = (uint32_t)ph.max_block; j.linked = ph.info.blockMode == LZ4F_blockLinked; j.block_checksum = ph.info.blockChecksumFlag != 0;
        j.content_checksum = ph.info.contentChecksumFlag != 0;
        const uint64_t by_dst = dstCapacity / ph.max_block + 2;
        const uint64_t by_src = frameCapacity / 5 + 2;                // every block costs at least 5 frame bytes
        uint64_t mb = by_dst < by_src ? by_dst : by_src;
        if (mb > 0x7FFFFFFFull) mb = 0x7FFFFFFFull;
        j.max_blocks = (uint32_t)mb;
        // a trailer (frame_dev.cuh): where it says the size words are, and the sequence index.  Only as hints: the kernels check both
        if (may_trail && foot.magic == TR_FOOT && foot.n_blocks && foot.n_blocks <= j.max_blocks && foot.total >= 8 + sizeof(foot) && foot.total <= frameCapacity - hs) {
            const uint64_t at = frameCapacity - foot.total;
            const uint64_t list_at = (at + 8 + 15) & ~(uint64_t)15, n_list = ((uint64_t)foot.n_blocks + 1) & ~1ull, ix_at = list_at + n_list * 8;
            if (ix_at + sizeof(foot) <= frameCapacity) {
                j.hint_list = (const uint64_t*)((const uint8_t*)d_frame + list_at); j.hint_n = foot.n_blocks;      // (frame_cap stays the whole buffer: `at` is a claim)
                const uint64_t ix_bytes = frameCapacity - sizeof(foot) - ix_at;
                if (ix_bytes >= sizeof(IxHeader) && foot.total_seqs) { j.d_index = (void*)((const uint8_t*)d_frame + ix_at); j.index_size = (size_t)ix_bytes; j.ix_seqs = foot.total_seqs; j.ix_entries = foot.total_entries; }
            }
        }
    }
    return e->launch_decompress(j, d_result);
}

size_t lz4f_mi355x_dev_decompressBlocks(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_frame, size_t frameCapacity,
                                        const lz4f_mi355x_block* d_table, uint32_t n_blocks, const LZ4F_frameInfo_t* info,
                                        lz4f_mi355x_result* d_result)
{
    return lz4f_mi355x_dev_decompressBlocksIndexed(e, d_dst, dstCapacity, d_frame, frameCapacity, d_table, n_blocks, info, nullptr, 0, d_result);
}

// the batch's dictionary as the kernels take it: the last 64 KiB at most (dictSize 0: none; bytes without a pointer: a length without
// an end, which batch_begin's callers refuse as a null pointer)
static DictTail batch_dict_tail(const void* d_dict, size_t dictSize)
{
    DictTail t;
    t.len = (uint32_t)std::min<size_t>(dictSize, 65536);
    t.end = t.len && d_dict ? (const uint8_t*)d_dict + dictSize : nullptr;
    return t;
}

// `dict`: none, the call's one dictionary (its tail is all the decoders take), or a set, each frame with the member its slot or its
// header names (lz4f_mi355x_dev_decompressFrames_usingDictSet; d_slot may be NULL)
static size_t decompress_frames(lz4f_mi355x_engine* e, const BatchSpans& sp, lz4f_mi355x_result* d_results, const BatchDict& dict)
{
    const uint32_t n_frames = sp.n_frames;
    const DictTail& dc = dict.one;
    size_t r;
    if (batch_open(e, n_frames, "dev_decompressFrames", sp.d_src && sp.d_src_off && sp.d_dst && sp.d_dst_off && d_results && (dc.end || !dc.len), r)) return r;
    hipStream_t st = (hipStream_t)e->stream;
    // the block table: a frame of full blocks never needs more than window / 64 KiB + 1 entries, so this bound needs nothing read back
    const uint64_t table_cap = batch_table_cap(n_frames, sp.dstBytes / BF_SHARE);
    Carve ws{e->bframes};
    const size_t frames_at = ws.take((size_t)n_frames * sizeof(BatchFrame)), counts_at = ws.take((size_t)n_frames * 4), ctl_at = ws.take(256, 256);
    const size_t slots_at = dict.set ? ws.take((size_t)n_frames * 4, 4) : 0;     // (the set call's own: the frames' resolved slots)
    if (ws.ensure() || e->btable.ensure((size_t)table_cap * sizeof(BatchBlk))) return make_err(LZ4F_ERROR_allocation_failed);
    BatchFrame* frames = ws.at<BatchFrame>(frames_at);
    uint32_t* counts = ws.at<uint32_t>(counts_at);
    uint32_t* ctl = ws.at<uint32_t>(ctl_at);
    BatchBlk* table = (BatchBlk*)e->btable.p;
    const uint8_t* src = (const uint8_t*)sp.d_src; uint8_t* dst = (uint8_t*)sp.d_dst;
    constexpr int W = 4;
    const uint32_t g256 = (n_frames + 255) / 256, gw = (n_frames + W - 1) / W;
    // the six launches in the form F (the decoders' DICT): `hs` is the head kernel's set argument, `dcs` the decoders' dictionary
    auto launch = [&](auto form, auto hs, auto dcs) {
        constexpr int F = decltype(form)::value;
        hipLaunchKernelGGL(k_bf_head<F == BF_SET>, dim3(g256), dim3(256), 0, st, src, (uint64_t)sp.srcBytes, sp.d_src_off, (uint64_t)sp.dstBytes, sp.d_dst_off,
                           n_frames, frames, counts, hs);
        hipLaunchKernelGGL(k_batch_place<BatchFrame>, dim3(1), dim3(1024), 0, st, (const uint32_t*)counts, n_frames, frames, table_cap, ctl);
        hipLaunchKernelGGL(k_bf_table, dim3(g256), dim3(256), 0, st, src, (const BatchFrame*)frames, n_frames, table);
        hipLaunchKernelGGL((k_bf_blocks<W, F>), batch_grid(table_cap, W), dim3(64 * W), 0, st, src, dst, (const BatchFrame*)frames, n_frames, table,
                           (const uint32_t*)ctl, dcs);
        hipLaunchKernelGGL((k_bf_serial<W, F>), dim3(gw), dim3(64 * W), 0, st, src, dst, frames, n_frames, dcs);
        hipLaunchKernelGGL((k_bf_finish<W, F>), dim3(gw), dim3(64 * W), 0, st, src, dst, frames, n_frames, (const BatchBlk*)table, (ResultRec*)d_results,
                           e->sw.no_content_check ? 0u : 1u, dcs);
    };
    if (dict.set) {
        uint32_t* slots = ws.at<uint32_t>(slots_at);
        launch(std::integral_constant<int, BF_SET>{}, BfHeadSet<true>{dict.set->view, dict.d_slot, slots}, BfSet{dict.set->view, slots});
        return batch_end("dev_decompressFrames_usingDictSet");
    }
    // (a dictionary: the DICT instantiations, every block through the scalar-parse decoder)
    if (dc.len) launch(std::integral_constant<int, 1>{}, BfHeadSet<false>{}, dc);
    else launch(std::integral_constant<int, 0>{}, BfHeadSet<false>{}, dc);
    return batch_end("dev_decompressFrames");
}

size_t lz4f_mi355x_dev_decompressFrames(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                        void* d_dst, size_t dstBytes, const uint64_t* d_dst_off, lz4f_mi355x_result* d_results)
{
    return decompress_frames(e, BatchSpans{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off}, d_results, BatchDict{});
}
size_t lz4f_mi355x_dev_decompressFrames_usingDict(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                  void* d_dst, size_t dstBytes, const uint64_t* d_dst_off, lz4f_mi355x_result* d_results,
                                                  const void* d_dict, size_t dictSize)
{
    return decompress_frames(e, BatchSpans{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off}, d_results,
                             BatchDict{EncDict{batch_dict_tail(d_dict, dictSize)}});
}

size_t lz4f_mi355x_dev_measureFrames(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                     uint64_t* d_dst_off, lz4f_mi355x_result* d_results)
{
    size_t r;
    if (batch_open(e, n_frames, "dev_measureFrames", d_src && d_src_off && d_results, r)) return r;
    hipStream_t st = (hipStream_t)e->stream;
    // the block table: sized from the call's arguments alone; frames behind an overflow are measured a wave per frame
    const uint64_t table_cap = batch_table_cap(n_frames, srcBytes / MF_SHARE);
    Carve ws{e->mframes};
    const size_t frames_at = ws.take((size_t)n_frames * sizeof(MeasFrame)), wins_at = ws.take((size_t)n_frames * 8),
                 counts_at = ws.take((size_t)n_frames * 4), ctl_at = ws.take(256, 256);
    if (ws.ensure() || e->mtable.ensure((size_t)table_cap * sizeof(MeasBlk))) return make_err(LZ4F_ERROR_allocation_failed);
    MeasFrame* frames = ws.at<MeasFrame>(frames_at);
    uint64_t* wins = ws.at<uint64_t>(wins_at);
    uint32_t* counts = ws.at<uint32_t>(counts_at);
    uint32_t* ctl = ws.at<uint32_t>(ctl_at);
    MeasBlk* table = (MeasBlk*)e->mtable.p;
    const uint8_t* src = (const uint8_t*)d_src;
    constexpr int W = 4;
    const uint32_t g256 = (n_frames + 255) / 256, gw = (n_frames + W - 1) / W;
    hipLaunchKernelGGL(k_mf_head, dim3(g256), dim3(256), 0, st, src, (uint64_t)srcBytes, d_src_off, n_frames, frames, counts);
    hipLaunchKernelGGL(k_batch_place<MeasFrame>, dim3(1), dim3(1024), 0, st, (const uint32_t*)counts, n_frames, frames, table_cap, ctl);
    hipLaunchKernelGGL(k_mf_table, dim3(g256), dim3(256), 0, st, src, (const MeasFrame*)frames, n_frames, table);
    hipLaunchKernelGGL((k_mf_blocks<W>), batch_grid(table_cap, W), dim3(64 * W), 0, st, src, (const MeasFrame*)frames, n_frames, table, (const uint32_t*)ctl);
    hipLaunchKernelGGL((k_mf_serial<W>), dim3(gw), dim3(64 * W), 0, st, src, frames, n_frames);
    hipLaunchKernelGGL((k_mf_finish<W>), dim3(gw), dim3(64 * W), 0, st, (const MeasFrame*)frames, n_frames, (const MeasBlk*)table, (ResultRec*)d_results, wins);
    if (d_dst_off) hipLaunchKernelGGL(k_mf_scan, dim3(1), dim3(1024), 0, st, (const uint64_t*)wins, n_frames, d_dst_off);
    return batch_end("dev_measureFrames");
}

// the frames of a batch back to back (pack_batch.cuh): the scan, then the copy dealt by output bytes
size_t lz4f_mi355x_dev_packFrames(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                  const lz4f_mi355x_result* d_results, void* d_dst, size_t dstBytes, uint64_t* d_dst_off,
                                  unsigned flags, lz4f_mi355x_result* d_pack)
{
    size_t r;
    if (batch_open(e, n_frames, "dev_packFrames", d_src && d_src_off && d_results && d_dst && d_dst_off, r)) return r;
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    if (srcBytes && dstBytes && s0 < d0 + dstBytes && d0 < s0 + srcBytes) { set_last_error("dev_packFrames: d_dst overlaps d_src"); return make_err(LZ4F_ERROR_GENERIC); }
    if (e->pctl.ensure(256)) return make_err(LZ4F_ERROR_allocation_failed);
    uint32_t* ctl = (uint32_t*)e->pctl.p;
    hipStream_t st = (hipStream_t)e->stream;
    hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(1024), 0, st, (const ResultRec*)d_results, d_src_off, (uint64_t)srcBytes, n_frames, (uint8_t*)d_dst,
                       (uint64_t)dstBytes, d_dst_off, (uint32_t)(flags & LZ4F_MI355X_PACK_DIRECTORY), ctl, (ResultRec*)d_pack);
    // (the tiles of dstBytes output bytes, and one for the destination's shift: the most the copy can have)
    hipLaunchKernelGGL(k_pk_copy, batch_grid((uint64_t)dstBytes / PK_TILE + 2, 1, PK_GRID), dim3(PK_THREADS), 0, st, (const uint8_t*)d_src, d_src_off, n_frames,
                       (uint8_t*)d_dst, (const uint64_t*)d_dst_off, (const uint32_t*)ctl);
    return batch_end("dev_packFrames");
}

size_t lz4f_mi355x_dev_readPackDirectory(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_pack, size_t packBytes, uint64_t* d_src_off,
                                         lz4f_mi355x_result* d_result)
{
    size_t r;
    if (batch_open(e, n_frames, "dev_readPackDirectory", d_pack && d_src_off, r)) return r;
    hipLaunchKernelGGL(k_pk_readdir, dim3(1), dim3(1024), 0, (hipStream_t)e->stream, (const uint8_t*)d_pack, (uint64_t)packBytes, n_frames, d_src_off,
                       (ResultRec*)d_result);
    return batch_end("dev_readPackDirectory");
}

// the node list of a split call (split_batch.cuh), from the call's arguments alone: a node for every frame asked for, one more for every
// LZ4F_MI355X_SPLIT_SHARE bytes of the stream (skippable frames, magics inside payloads), and 64
static uint64_t sp_node_cap(uint32_t max_frames, uint64_t src_bytes)
{
    return std::min<uint64_t>((uint64_t)max_frames + src_bytes / LZ4F_MI355X_SPLIT_SHARE + 64, 0xFFFFFFF0ull);
}
// the doubling rounds that reach every node of a list of `cap`: 2^rounds >= cap
static uint32_t sp_rounds(uint64_t cap)
{
    uint32_t r = 0;
    while ((1ull << r) < cap) r++;
    return r;
}

// the frames of a concatenated stream (split_batch.cuh): candidates, order, list, extents and links, reachability, place; the serial walk behind
size_t lz4f_mi355x_dev_splitFrames(lz4f_mi355x_engine* e, const void* d_src, size_t srcBytes, uint32_t max_frames, uint64_t* d_src_off,
                                   lz4f_mi355x_result* d_split)
{
    size_t r;
    if (batch_open(e, max_frames, "dev_splitFrames", d_src && d_src_off, r)) return r;
    hipStream_t st = (hipStream_t)e->stream;
    const uint8_t* src = (const uint8_t*)d_src;
    if (e->sw.split_serial) {
        hipLaunchKernelGGL(k_split_serial, dim3(1), dim3(256), 0, st, src, (uint64_t)srcBytes, (const SpCtl*)nullptr, 1u, max_frames, d_src_off, (ResultRec*)d_split);
        return batch_end("dev_splitFrames");
    }
    const uint64_t chunks64 = std::max<uint64_t>(((uint64_t)srcBytes + SP_CHUNK - 1) / SP_CHUNK, 1);      // (an empty stream has its root too)
    if (chunks64 > 0x7FFFFFFFull) { set_last_error("dev_splitFrames: srcBytes too large"); return make_err(LZ4F_ERROR_srcSize_tooLarge); }
    const uint32_t n_chunks = (uint32_t)chunks64;
    const uint64_t cap = sp_node_cap(max_frames, srcBytes);
    Carve ws{e->split};
    const size_t bits_at = ws.take((size_t)n_chunks * (SP_CHUNK / 8), 16), counts_at = ws.take((size_t)n_chunks * 4, 16), ctl_at = ws.take(256, 256),
                 list_at = ws.take((size_t)cap * 8, 16), nodes_at = ws.take((size_t)cap * sizeof(SpNode), 16), ja_at = ws.take((size_t)cap * 4, 16),
                 jb_at = ws.take((size_t)cap * 4, 16), reach_at = ws.take((size_t)cap, 16);
    if (ws.ensure()) return make_err(LZ4F_ERROR_allocation_failed);
    uint32_t* counts = ws.at<uint32_t>(counts_at);
    SpCtl* ctl = ws.at<SpCtl>(ctl_at);
    uint64_t* list = ws.at<uint64_t>(list_at);
    SpNode* nodes = ws.at<SpNode>(nodes_at);
    uint32_t* jump[2] = {ws.at<uint32_t>(ja_at), ws.at<uint32_t>(jb_at)};
    uint8_t* reach = ws.at<uint8_t>(reach_at);
    const dim3 g_chunks = batch_grid(n_chunks, 1, PK_GRID), g_nodes = batch_grid(cap, 256);
    hipLaunchKernelGGL(k_sp_cand, g_chunks, dim3(SP_THREADS), 0, st, src, (uint64_t)srcBytes, n_chunks, ws.at<uint16_t>(bits_at), counts);
    hipLaunchKernelGGL(k_sp_order, dim3(1), dim3(1024), 0, st, counts, n_chunks, (uint32_t)cap, ctl);
    hipLaunchKernelGGL(k_sp_list, g_chunks, dim3(SP_THREADS), 0, st, (const uint64_t*)ws.at<uint64_t>(bits_at), (const uint32_t*)counts, n_chunks, (const SpCtl*)ctl, list);
    hipLaunchKernelGGL(k_sp_extent, g_nodes, dim3(256), 0, st, src, (uint64_t)srcBytes, (const SpCtl*)ctl, (const uint64_t*)list, nodes, jump[0], reach);
    const uint32_t rounds = sp_rounds(cap);
    for (uint32_t r = 0; r < rounds; r++)
        hipLaunchKernelGGL(k_sp_double, g_nodes, dim3(256), 0, st, (const SpCtl*)ctl, (const uint32_t*)jump[r & 1], jump[(r & 1) ^ 1], reach);
    hipLaunchKernelGGL(k_sp_place, dim3(1), dim3(1024), 0, st, src, (uint64_t)srcBytes, ctl, (const uint64_t*)list, (const SpNode*)nodes, (const uint8_t*)reach,
                       max_frames, d_src_off, (ResultRec*)d_split);
    hipLaunchKernelGGL(k_split_serial, dim3(1), dim3(256), 0, st, src, (uint64_t)srcBytes, (const SpCtl*)ctl, 0u, max_frames, d_src_off, (ResultRec*)d_split);
    return batch_end("dev_splitFrames");
}

// a dictionary trained from the samples of a batch (train_dict.cuh): the corpus gathered, hashed and counted, the look-back, then
// `rounds` times the picks and their commit - the ladder is the parameters', never the samples'
size_t lz4f_mi355x_dev_trainDict(lz4f_mi355x_engine* e, uint32_t n_samples, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                 void* d_dict, size_t dictSize, const lz4f_mi355x_train_params* params, lz4f_mi355x_result* d_result)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    TdArgs a{LZ4F_MI355X_TRAIN_K, LZ4F_MI355X_TRAIN_D, LZ4F_MI355X_TRAIN_F, LZ4F_MI355X_TRAIN_ROUNDS};
    if (params) {
        if (params->k) a.k = params->k;
        if (params->d) a.d = params->d;
        if (params->f) a.f = params->f;
        if (params->rounds) a.rounds = params->rounds;
    }
    auto refuse = [](const char* what) { set_last_error("dev_trainDict: %s", what); return make_err(LZ4F_ERROR_GENERIC); };
    if (a.d != 4 && a.d != 6 && a.d != 8) return refuse("d must be 4, 6 or 8");
    if (a.k < a.d || a.k > TD_MAX_K) return refuse("k must be in [d, 4096]");
    if (a.f < 16 || a.f > 22) return refuse("f must be in [16, 22]");
    if (a.rounds < 1 || a.rounds > 64) return refuse("rounds must be in [1, 64]");
    if (dictSize > 65536) return refuse("dictSize above 64 KiB (LZ4 never reads further back)");
    if ((uint64_t)srcBytes >= (1ull << 31)) { set_last_error("dev_trainDict: srcBytes too large"); return make_err(LZ4F_ERROR_srcSize_tooLarge); }
    if (n_samples == 0 || dictSize == 0) return 0;
    if (const size_t r = batch_begin(e, "dev_trainDict", d_src && d_src_off && d_dict)) return r;
    hipStream_t st = (hipStream_t)e->stream;
    const uint32_t dict_size = (uint32_t)dictSize, epochs = std::max<uint32_t>(dict_size / a.k, 1);
    Carve ws{e->train};
    const size_t ctl_at = ws.take(256, 256), at_at = ws.take(((size_t)n_samples + 1) * 8, 16), c_at = ws.take(srcBytes + 32, 16),
                 hv_at = ws.take(srcBytes * 4 + 16, 16), back_at = ws.take(srcBytes * 2 + 16, 16), freq_at = ws.take((size_t)4 << a.f, 16),
                 best_at = ws.take((size_t)epochs * 8, 16);                              // (the counts and the picks lie together: one fill clears both)
    if (ws.ensure()) return make_err(LZ4F_ERROR_allocation_failed);
    TdCtl* ctl = ws.at<TdCtl>(ctl_at);
    uint64_t* at = ws.at<uint64_t>(at_at);
    uint8_t* C = ws.at<uint8_t>(c_at);
    uint32_t* hv = ws.at<uint32_t>(hv_at);
    uint16_t* back = ws.at<uint16_t>(back_at);
    uint32_t* freq = ws.at<uint32_t>(freq_at);
    unsigned long long* best = ws.at<unsigned long long>(best_at);
    const uint8_t* src = (const uint8_t*)d_src; uint8_t* dict = (uint8_t*)d_dict;
    HIP_TRY(hipMemsetAsync(freq, 0, ws.end - freq_at, st));
    const dim3 g_tiles = batch_grid((uint64_t)srcBytes + 1, TD_TILE);
    hipLaunchKernelGGL(k_td_scan, dim3(1), dim3(1024), 0, st, d_src_off, (uint64_t)srcBytes, n_samples, a, dict, dict_size, at, ctl, (ResultRec*)d_result);
    hipLaunchKernelGGL(k_td_gather, g_tiles, dim3(TD_THREADS), 0, st, src, d_src_off, n_samples, (const uint64_t*)at, (const TdCtl*)ctl, C);
    hipLaunchKernelGGL(k_td_hash, g_tiles, dim3(TD_THREADS), 0, st, (const uint8_t*)C, (const TdCtl*)ctl, a, hv, freq);
    hipLaunchKernelGGL(k_td_back, g_tiles, dim3(TD_THREADS), 0, st, (const uint32_t*)hv, (const TdCtl*)ctl, back);
    for (uint32_t r = 0; r < a.rounds; r++) {
        hipLaunchKernelGGL(k_td_pick, g_tiles, dim3(TD_THREADS), 0, st, (const uint32_t*)hv, (const uint16_t*)back, (const uint32_t*)freq, (const TdCtl*)ctl, best);
        hipLaunchKernelGGL(k_td_commit, dim3(1), dim3(TD_THREADS), 0, st, (const uint8_t*)C, (const uint32_t*)hv, (const uint16_t*)back, freq, ctl, best, a,
                           r + 1 == a.rounds ? 1u : 0u, dict, dict_size, (ResultRec*)d_result);
    }
    return batch_end("dev_trainDict");
}

// `dict`: the call's dictionary - none, one (a raw one's tail, or a prepared one's with its digests), or a set, frame i with the
// member d_slot[i] names (lz4f_mi355x_dev_compressFrames_usingDictSet)
static size_t compress_frames(lz4f_mi355x_engine* e, const BatchSpans& sp, const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_results,
                              const BatchDict& dict)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    const uint32_t n_frames = sp.n_frames;
    LZ4F_preferences_t p; size_t bs;
    const size_t bad_prefs = resolve_prefs(prefs, p, bs);
    // Of a level the dictionary does not serve and a block size that does not exist, the one-dictionary calls report the block size,
    // the set call the level: it always judged its set against the level in front of the preferences
    if (bad_prefs && !dict.set) return bad_prefs;
    // (levels 3-12 take a dictionary only with the hash-chain digest: seeding a raw one costs up to 69 barrier rounds in front of
    // every chunk.  Nothing is enqueued)
    if (dict.any() && p.compressionLevel >= 3 && !dict.serves_hc()) {
        set_last_error(dict.set ? "dev_compressFrames_usingDictSet: levels 3-12 take only members made by dev_createCDictHC"
                                : "dev_compressFrames_usingDict: levels 3-12 take a dictionary only as a CDict of dev_createCDictHC");
        return make_err(LZ4F_ERROR_compressionLevel_invalid);
    }
    if (bad_prefs) return bad_prefs;
    if (n_frames == 0) return 0;
    const EncDict& dc = dict.one;
    if (const size_t r = batch_begin(e, "dev_compressFrames", sp.d_src && sp.d_src_off && sp.d_dst && sp.d_dst_off && d_results && (dc.end || !dc.len) &&
                                                              (dict.d_slot || !dict.set))) return r;
    hipStream_t st = (hipStream_t)e->stream;
    // what the frames have in common; the header is each frame's own (k_bc_frames: frame_head_write with its content size)
    const LZ4F_frameInfo_t& f = p.frameInfo;
    BcPrefs pf; memset(&pf, 0, sizeof(pf));
    pf.block_size = (uint32_t)bs; pf.bsid = (uint32_t)f.blockSizeID; pf.linked = f.blockMode == LZ4F_blockLinked; pf.block_checksum = f.blockChecksumFlag != 0;
    pf.content_checksum = f.contentChecksumFlag != 0; pf.content_size = f.contentSize != 0; pf.dict_id = f.dictID;
    const bool hc = p.compressionLevel >= 3;                           // (the deterministic finders whatever the engine's switch says)
    if (hc) { const HcLevel hl = hc_level_of(p.compressionLevel, e->sw); pf.hc_attempts = hl.attempts; pf.hc_lazy = hl.lazy; }
    // the tables and the pool, from the call's arguments alone: chunks are 64 KiB whatever the block size (pick_chunk_size), so spans
    // that do not overlap have at most n_frames + srcBytes / 64 KiB chunks, no more blocks, and a record per 4 bytes + one per chunk
    const uint64_t cap = batch_table_cap(n_frames, sp.srcBytes / BC_CHUNK);
    const uint64_t rec_cap = (uint64_t)sp.srcBytes / 4 + cap;
    Carve ws{e->cframes};
    const size_t frames_at = ws.take((size_t)n_frames * sizeof(BcFrame)), ctl_at = ws.take(256, 256);
    const size_t recs_had = e->recs.cap;
    if (ws.ensure() || e->cblocks.ensure((size_t)cap * sizeof(BcBlk)) || e->cchunks.ensure((size_t)cap * sizeof(BcChunk)) ||
        e->info.ensure((size_t)cap * sizeof(ChunkInfo)) || e->recs.ensure(64 + (size_t)rec_cap * 8))
        return make_err(LZ4F_ERROR_allocation_failed);
    if (e->recs.cap != recs_had) e->recs_ctl_clean = nullptr;          // (a new pool: the single call's control words in its first 64 bytes are not zero yet)
    BcFrame* frames = ws.at<BcFrame>(frames_at);
    uint32_t* ctl = ws.at<uint32_t>(ctl_at);
    BcBlk* blocks = (BcBlk*)e->cblocks.p;
    BcChunk* chunks = (BcChunk*)e->cchunks.p;
    ChunkInfo* info = (ChunkInfo*)e->info.p;
    // The pool lies behind the single call's control words, which stay as they are (recs_ctl_clean).  It does overwrite the single
    // call's per-chunk list offsets (rec_offs) and `info`: both are a call's own - every single-call finder writes the offset and the
    // ChunkInfo of every chunk it later reads before anything reads them, and nothing is carried from one call to the next.
    uint64_t* pool = (uint64_t*)e->recs.p + 8;
    const uint8_t* src = (const uint8_t*)sp.d_src; uint8_t* dst = (uint8_t*)sp.d_dst;
    constexpr int W = 4;
    const uint32_t g256 = (n_frames + 255) / 256, gw = (n_frames + W - 1) / W;
    const dim3 g_ent = batch_grid(cap, W);                             // (a wave per entry, striding over the entries in use)
    // the launches, for a dictionary source D (the finders' last argument): `head` with its set arguments, and k_bc_frames' set argument
    auto launch = [&](const auto& dcs, auto fs, auto head, auto... head_set) {
        constexpr bool SET = std::is_same<decltype(fs), BcFramesSet<true>>::value;
        const auto find = bc_finder(hc, dcs);
        hipLaunchKernelGGL(head, dim3(g256), dim3(256), 0, st, (uint64_t)sp.srcBytes, sp.d_src_off, (uint64_t)sp.dstBytes, sp.d_dst_off, n_frames, pf, frames,
                           head_set...);
        hipLaunchKernelGGL(k_bc_place, dim3(1), dim3(1024), 0, st, frames, n_frames, cap, cap, rec_cap, ctl);
        hipLaunchKernelGGL((k_bc_table<W>), dim3(gw), dim3(64 * W), 0, st, (const BcFrame*)frames, n_frames, pf, blocks, chunks);
        hipLaunchKernelGGL(find.kernel, batch_grid(cap, 1, find.most_wgs), dim3(find.threads), 0, st, src, (const BcFrame*)frames, n_frames, (const BcChunk*)chunks,
                           (const uint32_t*)ctl, info, pool, pf, dcs);
        hipLaunchKernelGGL((k_bc_layout<W>), g_ent, dim3(64 * W), 0, st, (const BcFrame*)frames, n_frames, blocks, (const uint32_t*)ctl, info);
        hipLaunchKernelGGL((k_bc_frames<W, SET>), dim3(gw), dim3(64 * W), 0, st, dst, frames, n_frames, pf, blocks, info, (ResultRec*)d_results, fs);
        hipLaunchKernelGGL((k_bc_emit<W>), g_ent, dim3(64 * W), 0, st, src, dst, (const BcFrame*)frames, n_frames, (const BcChunk*)chunks, (const uint32_t*)ctl,
                           (const ChunkInfo*)info, (const uint64_t*)pool);
        if (pf.block_checksum) {
            if (bs > (256u << 10))                                     // (few big blocks: the four-lane chain, as the single call's k_xxh32_blocks4)
                hipLaunchKernelGGL((k_bc_blockck<W, true>), g_ent, dim3(64 * W), 0, st, dst, (const BcFrame*)frames, n_frames, (const BcBlk*)blocks, (const uint32_t*)ctl);
            else
                hipLaunchKernelGGL((k_bc_blockck<W, false>), g_ent, dim3(64 * W), 0, st, dst, (const BcFrame*)frames, n_frames, (const BcBlk*)blocks, (const uint32_t*)ctl);
        }
        if (pf.content_checksum) hipLaunchKernelGGL((k_bc_content<W>), dim3(gw), dim3(64 * W), 0, st, src, dst, (const BcFrame*)frames, n_frames);
    };
    // (a set: head, finder and header writer in their set forms)
    if (dict.set) launch(dict.set->view, BcFramesSet<true>{dict.set->view}, k_bc_head_set, dict.d_slot, dict.set->view.count);
    else launch(dc, BcFramesSet<false>{}, k_bc_head);
    return batch_end("dev_compressFrames");
}

size_t lz4f_mi355x_dev_compressFrames(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                      void* d_dst, size_t dstBytes, const uint64_t* d_dst_off, const LZ4F_preferences_t* prefs,
                                      lz4f_mi355x_result* d_results)
{
    return compress_frames(e, BatchSpans{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off}, prefs, d_results, BatchDict{});
}
size_t lz4f_mi355x_dev_compressFrames_usingDict(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                void* d_dst, size_t dstBytes, const uint64_t* d_dst_off, const LZ4F_preferences_t* prefs,
                                                lz4f_mi355x_result* d_results, const void* d_dict, size_t dictSize)
{
    return compress_frames(e, BatchSpans{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off}, prefs, d_results,
                           BatchDict{EncDict{batch_dict_tail(d_dict, dictSize)}});
}

// ---- the prepared dictionary: the dictionary's last 64 KiB, owned, and the finder's table seeded from them once (createCDictHC: the
// hash-chain finder's head and chain too) ----
// `hc`: with the hash-chain finder's digest between the solo digest and the copy (`who`: the call's name in messages)
static size_t create_cdict(lz4f_mi355x_engine* e, lz4f_mi355x_cdict** out, const void* d_dict, size_t dictSize, bool hc, const char* who)
{
    if (out) *out = nullptr;
    if (!e || !out || (!d_dict && dictSize)) { set_last_error("%s: null pointer", who); return make_err(LZ4F_ERROR_GENERIC); }
    if (hipSetDevice(e->device) != hipSuccess) { set_last_error("hipSetDevice failed"); return make_err(LZ4F_ERROR_GENERIC); }
    lz4f_mi355x_cdict* c = new (std::nothrow) lz4f_mi355x_cdict();
    if (!c) { set_last_error("%s: out of memory", who); return make_err(LZ4F_ERROR_allocation_failed); }
    c->engine = e; c->hc = hc;
    const DictTail src = batch_dict_tail(d_dict, dictSize);
    if (src.len) {
        // one allocation: the digests (16-byte aligned: they lead, and both are whole vectors), then the copy
        void* p = nullptr;
        const size_t hc_bytes = hc ? hc_digest_bytes(src.len) : 0, bytes = SOLO_DIGEST_BYTES + hc_bytes + (size_t)src.len;
        const hipError_t he = hipMalloc(&p, bytes);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            set_last_error("%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(he));
            delete c;
            return make_err(LZ4F_ERROR_allocation_failed);
        }
        uint8_t* data = (uint8_t*)p + SOLO_DIGEST_BYTES + hc_bytes;
        uint4* solo_digest = (uint4*)p, * hc_digest = hc ? (uint4*)((uint8_t*)p + SOLO_DIGEST_BYTES) : nullptr;
        c->mem = p; c->dict.end = data + src.len; c->dict.len = src.len; c->dict.solo_digest = solo_digest; c->dict.hc_digest = hc_digest;
        hipStream_t st = (hipStream_t)e->stream;
        if (hipMemcpyAsync(data, src.end - src.len, src.len, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            (void)hipGetLastError(); (void)hipFree(p); delete c;
            set_last_error("%s: the dictionary's copy failed", who);
            return make_err(LZ4F_ERROR_GENERIC);
        }
        hipLaunchKernelGGL(k_solo_digest_dict, dim3(1), dim3(64), 0, st, c->dict.end, c->dict.len, solo_digest);
        if (hc) hipLaunchKernelGGL(k_hc_digest_dict, dim3(1), dim3(64 * HC_WAVES), 0, st, c->dict.end, c->dict.len, hc_digest);
        if (hipGetLastError() != hipSuccess) {                             // (the copy may be in flight: wait before its target goes)
            (void)hipStreamSynchronize(st); (void)hipFree(p); delete c;
            set_last_error("%s: launch failed", who);
            return make_err(LZ4F_ERROR_GENERIC);
        }
    }
    *out = c;
    return 0;
}

size_t lz4f_mi355x_dev_createCDict(lz4f_mi355x_engine* e, lz4f_mi355x_cdict** out, const void* d_dict, size_t dictSize)
{
    return create_cdict(e, out, d_dict, dictSize, false, "dev_createCDict");
}
size_t lz4f_mi355x_dev_createCDictHC(lz4f_mi355x_engine* e, lz4f_mi355x_cdict** out, const void* d_dict, size_t dictSize)
{
    return create_cdict(e, out, d_dict, dictSize, true, "dev_createCDictHC");
}
int lz4f_mi355x_cdict_has_hc(const lz4f_mi355x_cdict* c) { return c && c->hc ? 1 : 0; }

// a device allocation that kernels on its engine's stream may still read goes: the stream's work first, then the memory (which goes
// even when the wait failed).  `who`: the call's name in the message
static size_t free_behind_stream(const lz4f_mi355x_engine* e, void* mem, const char* who)
{
    if (!mem) return 0;                                                    // (an empty one owns nothing and has nothing in flight)
    size_t r = 0;
    if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize((hipStream_t)e->stream) != hipSuccess) {
        (void)hipGetLastError(); set_last_error("%s: waiting for the engine's stream failed", who); r = make_err(LZ4F_ERROR_GENERIC);
    }
    (void)hipFree(mem);
    return r;
}

size_t lz4f_mi355x_dev_freeCDict(lz4f_mi355x_cdict* c)
{
    if (!c) return 0;
    const size_t r = free_behind_stream(c->engine, c->mem, "dev_freeCDict");
    delete c;
    return r;
}

const void* lz4f_mi355x_cdict_data(const lz4f_mi355x_cdict* c, size_t* size)
{
    if (size) *size = c ? c->dict.len : 0;
    return c && c->dict.len ? c->dict.end - c->dict.len : nullptr;
}

size_t lz4f_mi355x_dev_compressFrames_usingCDict(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                 void* d_dst, size_t dstBytes, const uint64_t* d_dst_off, const LZ4F_preferences_t* prefs,
                                                 lz4f_mi355x_result* d_results, const lz4f_mi355x_cdict* cdict)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    const BatchSpans sp{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off};
    if (!cdict || !cdict->dict.len) return compress_frames(e, sp, prefs, d_results, BatchDict{});
    if (cdict->engine != e) { set_last_error("dev_compressFrames_usingCDict: cdict belongs to another engine"); return make_err(LZ4F_ERROR_GENERIC); }
    // (a dictionary of 1-3 bytes: the finder ignores it, its digest is the cleared table - the _usingDict kernel, as that call launches it)
    EncDict dc = cdict->dict;
    if (dc.len < 4) dc.solo_digest = dc.hc_digest = nullptr;
    return compress_frames(e, sp, prefs, d_results, BatchDict{dc, cdict->hc});
}

// ---- a set of prepared dictionaries: one chosen per frame, by slot or by the header's dictID (dictset.cuh) ----
size_t lz4f_mi355x_dev_createDictSet(lz4f_mi355x_engine* e, lz4f_mi355x_dictset** out, uint32_t n_dicts, const lz4f_mi355x_cdict* const* cdicts,
                                     const uint32_t* dictIDs)
{
    if (out) *out = nullptr;
    if (!e || !out || (n_dicts && (!cdicts || !dictIDs))) { set_last_error("dev_createDictSet: null pointer"); return make_err(LZ4F_ERROR_GENERIC); }
    if (n_dicts > DS_MOST) { set_last_error("dev_createDictSet: %u members (at most %u)", n_dicts, DS_MOST); return make_err(LZ4F_ERROR_GENERIC); }
    // the IDs in order, each with its member: pairwise distinct, or the lookup has no answer
    std::vector<std::pair<uint32_t, uint32_t>> by_id;
    std::vector<DsMember> members;
    try { by_id.resize(n_dicts); members.resize(n_dicts); }
    catch (const std::bad_alloc&) { set_last_error("dev_createDictSet: out of memory"); return make_err(LZ4F_ERROR_allocation_failed); }
    bool all_hc = true;
    for (uint32_t k = 0; k < n_dicts; k++) {
        const lz4f_mi355x_cdict* c = cdicts[k];
        if (c && c->engine != e) { set_last_error("dev_createDictSet: member %u belongs to another engine", k); return make_err(LZ4F_ERROR_GENERIC); }
        DsMember m{nullptr, nullptr, nullptr, 0u, dictIDs[k]};
        if (c && c->dict.len) {
            m.end = c->dict.end; m.len = c->dict.len;
            if (m.len >= 4) { m.solo_digest = c->dict.solo_digest; m.hc_digest = c->dict.hc_digest; }      // (1-3 bytes: the finders ignore it)
            if (!c->hc) all_hc = false;
        }
        members[k] = m;
        by_id[k] = {dictIDs[k], k};
    }
    std::sort(by_id.begin(), by_id.end());
    for (uint32_t k = 1; k < n_dicts; k++)
        if (by_id[k].first == by_id[k - 1].first) {
            set_last_error("dev_createDictSet: duplicate dictID %u (members %u and %u)", by_id[k].first, by_id[k - 1].second, by_id[k].second);
            return make_err(LZ4F_ERROR_GENERIC);
        }
    if (hipSetDevice(e->device) != hipSuccess) { set_last_error("hipSetDevice failed"); return make_err(LZ4F_ERROR_GENERIC); }
    lz4f_mi355x_dictset* s = new (std::nothrow) lz4f_mi355x_dictset();
    if (!s) { set_last_error("dev_createDictSet: out of memory"); return make_err(LZ4F_ERROR_allocation_failed); }
    s->engine = e; s->all_hc = all_hc;
    if (n_dicts) {
        const size_t members_bytes = (size_t)n_dicts * sizeof(DsMember), bytes = members_bytes + (size_t)n_dicts * 8;
        std::vector<uint8_t>& host = s->staged;
        try { host.resize(bytes); } catch (const std::bad_alloc&) { delete s; set_last_error("dev_createDictSet: out of memory"); return make_err(LZ4F_ERROR_allocation_failed); }
        memcpy(host.data(), members.data(), members_bytes);
        uint32_t* ids = (uint32_t*)(host.data() + members_bytes), * order = ids + n_dicts;
        for (uint32_t k = 0; k < n_dicts; k++) { ids[k] = by_id[k].first; order[k] = by_id[k].second; }
        void* p = nullptr;
        const hipError_t he = hipMalloc(&p, bytes);
        if (he != hipSuccess) {
            (void)hipGetLastError(); delete s;
            set_last_error("dev_createDictSet: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(he));
            return make_err(LZ4F_ERROR_allocation_failed);
        }
        // (ordered on the stream in front of the set's first use; `host` lives as long as the set)
        if (hipMemcpyAsync(p, host.data(), bytes, hipMemcpyHostToDevice, (hipStream_t)e->stream) != hipSuccess) {
            (void)hipGetLastError(); (void)hipStreamSynchronize((hipStream_t)e->stream); (void)hipFree(p); delete s;
            set_last_error("dev_createDictSet: the table's upload failed");
            return make_err(LZ4F_ERROR_GENERIC);
        }
        s->mem = p;
        s->view.members = (const DsMember*)p; s->view.ids = (const uint32_t*)((uint8_t*)p + members_bytes); s->view.order = s->view.ids + n_dicts;
        s->view.count = n_dicts;
    }
    *out = s;
    return 0;
}

size_t lz4f_mi355x_dev_freeDictSet(lz4f_mi355x_dictset* s)
{
    if (!s) return 0;
    const size_t r = free_behind_stream(s->engine, s->mem, "dev_freeDictSet");
    delete s;
    return r;
}

uint32_t lz4f_mi355x_dictset_count(const lz4f_mi355x_dictset* s) { return s ? s->view.count : 0u; }

// the set of a set call: there, and this engine's
static size_t check_dictset(const lz4f_mi355x_engine* e, const lz4f_mi355x_dictset* set, const char* who)
{
    if (!set) { set_last_error("%s: null dictset", who); return make_err(LZ4F_ERROR_GENERIC); }
    if (set->engine != e) { set_last_error("%s: dictset belongs to another engine", who); return make_err(LZ4F_ERROR_GENERIC); }
    return 0;
}

size_t lz4f_mi355x_dev_resolveDictIDs(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                      const lz4f_mi355x_dictset* set, uint32_t* d_slot)
{
    size_t r;
    if (batch_idle(e, n_frames, r) || (r = check_dictset(e, set, "dev_resolveDictIDs")) != 0) return r;
    if ((r = batch_begin(e, "dev_resolveDictIDs", d_src && d_src_off && d_slot)) != 0) return r;
    hipLaunchKernelGGL(k_ds_resolve, dim3((n_frames + 255) / 256), dim3(256), 0, (hipStream_t)e->stream, (const uint8_t*)d_src, (uint64_t)srcBytes, d_src_off,
                       n_frames, set->view, d_slot);
    return batch_end("dev_resolveDictIDs");
}

size_t lz4f_mi355x_dev_compressFrames_usingDictSet(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                   void* d_dst, size_t dstBytes, const uint64_t* d_dst_off, const LZ4F_preferences_t* prefs,
                                                   lz4f_mi355x_result* d_results, const lz4f_mi355x_dictset* set, const uint32_t* d_slot)
{
    // (a set call of no frames returns before its set, its preferences and the level are looked at; the one-dictionary calls judge theirs first)
    size_t r;
    if (batch_idle(e, n_frames, r) || (r = check_dictset(e, set, "dev_compressFrames_usingDictSet")) != 0) return r;
    return compress_frames(e, BatchSpans{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off}, prefs, d_results, BatchDict{EncDict{}, false, set, d_slot});
}

size_t lz4f_mi355x_dev_decompressFrames_usingDictSet(lz4f_mi355x_engine* e, uint32_t n_frames, const void* d_src, size_t srcBytes,
                                                     const uint64_t* d_src_off, void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                     lz4f_mi355x_result* d_results, const lz4f_mi355x_dictset* set, const uint32_t* d_slot)
{
    size_t r;
    if (batch_idle(e, n_frames, r) || (r = check_dictset(e, set, "dev_decompressFrames_usingDictSet")) != 0) return r;
    return decompress_frames(e, BatchSpans{n_frames, d_src, srcBytes, d_src_off, d_dst, dstBytes, d_dst_off}, d_results, BatchDict{EncDict{}, false, set, d_slot});
}

size_t lz4f_mi355x_dev_xxh32(lz4f_mi355x_engine* e, const void* d_base, const uint64_t* d_off, const uint32_t* d_len, uint32_t n_blocks, uint32_t* d_out)
{
    if (!e) return make_err(LZ4F_ERROR_GENERIC);
    if (hipSetDevice(e->device) != hipSuccess) { set_last_error("hipSetDevice failed"); return make_err(LZ4F_ERROR_GENERIC); }
    if (n_blocks == 0) return 0;
    constexpr int W = 4;
    hipLaunchKernelGGL((k_xxh32_ranges<W>), dim3((n_blocks + W - 1) / W), dim3(64 * W), 0, (hipStream_t)e->stream, (const uint8_t*)d_base, d_off, d_len,
                       n_blocks, d_out);
    if (hipGetLastError() != hipSuccess) { set_last_error("xxh32 launch failed"); return make_err(LZ4F_ERROR_GENERIC); }
    return 0;
}

// developer aid (tests/test_gpu_e1_merge.py; not in the header): pass E1's merge of one tile, either form (0: before round 7, 1: E1_V9), on
// caller-given device buffers - s_end[512] and s_n[512] (the per-slice words), lists (512 x 32 records, as the search leaves them), a
// record workspace for n_chunks chunks and a pool of rec_pool records (8 * (rec_pool_at(n_chunks) + rec_pool) bytes), n_chunks ChunkInfo
// and the mode word.  Runs on the device's null stream and waits.  0: done; 1: an argument is out of range; 2: a HIP error
__attribute__((visibility("default"))) int lz4f_mi355x_debug_e1_merge(int form, const uint32_t* d_s_end, const uint8_t* d_s_n, const uint64_t* d_lists, uint32_t n_chunks,
                                                                      uint64_t rec_pool, uint32_t c, uint32_t ts, uint32_t te, uint32_t bend, uint32_t nslice, void* d_info,
                                                                      uint64_t* d_recs, uint32_t* d_mode)
{
    if ((form != 0 && form != 1) || !d_s_end || !d_s_n || !d_lists || !d_info || !d_recs || !d_mode) return 1;
    if (c >= n_chunks || nslice > E1_NSLICE || te < ts || te - ts > E1_TILE || (uint64_t)nslice * E1_SLICE < te - ts || bend < te || ts > 0x7FFF0000u) return 1;
    EncGeom g{}; g.n_chunks = n_chunks; g.rec_pool = rec_pool;
    if (form) hipLaunchKernelGGL((k_e1_merge_probe<1>), dim3(1), dim3(64), 0, 0, d_s_end, d_s_n, d_lists, g, c, ts, te, bend, nslice, (ChunkInfo*)d_info, d_recs, d_mode);
    else      hipLaunchKernelGGL((k_e1_merge_probe<0>), dim3(1), dim3(64), 0, 0, d_s_end, d_s_n, d_lists, g, c, ts, te, bend, nslice, (ChunkInfo*)d_info, d_recs, d_mode);
    return (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess) ? 0 : 2;
}

// developer aid (tests/test_gpu_spx_index.py; not in the header): the unchanged k_spx_index on caller-given device bytes - d_frame[0, frame_cap)
// with n blocks (src_off, word) in it, the size word's top bit a stored block as in the frame.  not_dense / bytes_per_seq: the two words of
// k_density_probe the kernel reads (both null: no only_if, as under LZ4F_MI355X_NO_DENSITY_PROBE).  pt_fill: the word every point of the
// workspace holds before the launch.  Copied back to the host: cnt, osz, nr (n words each), points (n rows of SPX_MAXPT + 1 points of three
// words: a block's nr + 1 points lead its row, the rest keeps pt_fill), ctl[0] = IxCtl::gave_up, ctl[1] = IxCtl::spx_stitched.  Runs on the
// device's null stream and waits.  0: done; 1: an argument is out of range; 2: a HIP error
__attribute__((visibility("default"))) int lz4f_mi355x_debug_spx_index(const uint8_t* d_frame, uint64_t frame_cap, uint32_t n, const uint64_t* src_off, const uint32_t* word,
                                                                      const uint32_t* not_dense, const uint32_t* bytes_per_seq, uint32_t pt_fill, uint32_t* cnt, uint32_t* osz,
                                                                      uint32_t* nr, uint32_t* points, uint32_t* ctl)
{
    if (!d_frame || !src_off || !word || !cnt || !osz || !nr || !points || !ctl || n == 0 || n > 4096 || frame_cap > (1ull << 40)) return 1;
    if ((not_dense == nullptr) != (bytes_per_seq == nullptr)) return 1;
    for (uint32_t b = 0; b < n; b++) if (src_off[b] > frame_cap) return 1;
    const size_t row = (size_t)(SPX_MAXPT + 1) * sizeof(SpxPoint), at_tbl = sizeof(IxCtl), at_res = at_tbl + (size_t)n * sizeof(BlockOut), at_dens = at_res + 64,
                 at_cnt = at_dens + 64, at_T = at_cnt + (((size_t)n * 12 + 63) & ~(size_t)63), total = at_T + (size_t)n * row;
    std::vector<uint8_t> h(at_T, 0);
    for (uint32_t b = 0; b < n; b++) { BlockOut e{src_off[b], 0, word[b], 0}; memcpy(&h[at_tbl + (size_t)b * sizeof(BlockOut)], &e, sizeof(e)); }
    ResultRec r{}; r.status = ST_OK; r.n_blocks = n; memcpy(&h[at_res], &r, sizeof(r));
    if (not_dense) { Density d{0, *not_dense, *bytes_per_seq}; memcpy(&h[at_dens], &d, sizeof(d)); }
    for (size_t i = at_cnt; i < at_T; i += 4) memcpy(&h[i], &pt_fill, 4);
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) return 2;
    bool ok = hipMemcpy(d, h.data(), at_T, hipMemcpyHostToDevice) == hipSuccess && hipMemsetD32((hipDeviceptr_t)(d + at_T), (int)pt_fill, (size_t)n * row / 4) == hipSuccess;
    if (ok) {
        uint32_t* dc = (uint32_t*)(d + at_cnt);
        hipLaunchKernelGGL(k_spx_index, dim3(n), dim3(SPX_MAXSEG), 0, 0, d_frame, frame_cap, (const BlockOut*)(d + at_tbl), (const ResultRec*)(d + at_res), n, dc, dc + n,
                           (SpxPoint*)(d + at_T), dc + 2 * (size_t)n, (IxCtl*)d, not_dense ? (const uint32_t*)&((const Density*)(d + at_dens))->not_dense : (const uint32_t*)nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    IxCtl c{};
    ok = ok && hipMemcpy(&c, d, offsetof(IxCtl, chain_total), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(cnt, d + at_cnt, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(osz, d + at_cnt + (size_t)n * 4, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(nr, d + at_cnt + (size_t)n * 8, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(points, d + at_T, (size_t)n * row, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    if (!ok) return 2;
    ctl[0] = c.gave_up; ctl[1] = c.spx_stitched;
    return 0;
}

}  // extern "C"
