/*
 * lz4f_mi355x.h -- C ABI of liblz4f_mi355x.so: the MI355X-native LZ4 frame codec that drops in
 * under Codec.Compression.LZ4.Conduit (nh2/lz4-frame-conduit).
 *
 * PART 1 is the drop-in boundary: exactly the twelve LZ4F_* entry points the reference's
 * inline-c FFI binds (citations are /root/reference/src/Codec/Compression/LZ4/Conduit.hsc),
 * with the struct layouts its Storable instances poke (CTypes.hsc:155-232).  The symbols are
 * exported under BOTH the upstream names (LZ4F_compressUpdate ...) so that swapping the cabal
 * `c-sources` for `extra-libraries: lz4f_mi355x` is the whole integration, and
 * under an lz4f_mi355x_ prefix (same functions) for processes that also load liblz4.
 * Every block is encoded / decoded / checksummed by HIP kernels on the GPU; there is no CPU
 * fallback: with no usable device the calls return ERROR_GENERIC (and lz4f_mi355x_last_error()
 * says why).
 *
 * PART 2 is the bulk extension the GPU needs (SURVEY.md section 8b "Bulk extension"): whole
 * frames / many blocks per call, host-pointer and device-pointer variants.
 */
#ifndef LZ4F_MI355X_H
#define LZ4F_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZ4F_MI355X_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------------
 * PART 1 -- the LZ4F-compatible streaming API (rows a1, a3, a6, a7 of SURVEY.md section 8a)
 * ------------------------------------------------------------------------------------------ */

#define LZ4F_VERSION          100   /* consumed at Conduit.hsc:199, :242, :568 */
#define LZ4F_HEADER_SIZE_MIN  7
#define LZ4F_HEADER_SIZE_MAX  19    /* consumed at Conduit.hsc:367, :466 */
#define LZ4F_BLOCK_HEADER_SIZE 4
#define LZ4F_BLOCK_CHECKSUM_SIZE 4
#define LZ4F_CONTENT_CHECKSUM_SIZE 4

typedef size_t LZ4F_errorCode_t;

/* CTypes.hsc:48-66 (BlockSizeID) */
typedef enum { LZ4F_default = 0, LZ4F_max64KB = 4, LZ4F_max256KB = 5, LZ4F_max1MB = 6, LZ4F_max4MB = 7 } LZ4F_blockSizeID_t;
/* CTypes.hsc:77-91 (BlockMode) */
typedef enum { LZ4F_blockLinked = 0, LZ4F_blockIndependent } LZ4F_blockMode_t;
/* CTypes.hsc:98-112 (ContentChecksum) */
typedef enum { LZ4F_noContentChecksum = 0, LZ4F_contentChecksumEnabled } LZ4F_contentChecksum_t;
/* CTypes.hsc:117-131 (BlockChecksum) */
typedef enum { LZ4F_noBlockChecksum = 0, LZ4F_blockChecksumEnabled } LZ4F_blockChecksum_t;
/* CTypes.hsc:136-150 (FrameType) */
typedef enum { LZ4F_frame = 0, LZ4F_skippableFrame } LZ4F_frameType_t;

/* CTypes.hsc:155-199 (FrameInfo): 32 bytes; offsets 0,4,8,12,16,24,28 */
typedef struct {
    LZ4F_blockSizeID_t     blockSizeID;
    LZ4F_blockMode_t       blockMode;
    LZ4F_contentChecksum_t contentChecksumFlag;
    LZ4F_frameType_t       frameType;
    unsigned long long     contentSize;
    unsigned               dictID;
    LZ4F_blockChecksum_t   blockChecksumFlag;
} LZ4F_frameInfo_t;

/* CTypes.hsc:202-232 (Preferences): 56 bytes; offsets 0,32,36,40,44 */
typedef struct {
    LZ4F_frameInfo_t frameInfo;
    int      compressionLevel;   /* <= 2: the fast encoder; 3..12: high compression (hash-chain search, lazy parse; equal input ->
                                    equal bytes); > 12 is 12.  favorDecSpeed is accepted and ignored.  The reference pins 0 (Conduit.hsc:260) */
    unsigned autoFlush;
    unsigned favorDecSpeed;
    unsigned reserved[3];
} LZ4F_preferences_t;

typedef struct { unsigned stableSrc; unsigned reserved[3]; } LZ4F_compressOptions_t;
typedef struct { unsigned stableDst; unsigned reserved[3]; } LZ4F_decompressOptions_t;

typedef struct LZ4F_cctx_s LZ4F_cctx;   /* CTypes.hsc:235 */
typedef struct LZ4F_dctx_s LZ4F_dctx;   /* CTypes.hsc:236 */

/* Error enum order == upstream lz4frame.h (names surface verbatim as "lz4frame error: <name>",
 * Conduit.hsc:160) */
typedef enum {
    LZ4F_OK_NoError = 0, LZ4F_ERROR_GENERIC, LZ4F_ERROR_maxBlockSize_invalid, LZ4F_ERROR_blockMode_invalid,
    LZ4F_ERROR_contentChecksumFlag_invalid, LZ4F_ERROR_compressionLevel_invalid, LZ4F_ERROR_headerVersion_wrong,
    LZ4F_ERROR_blockChecksum_invalid, LZ4F_ERROR_reservedFlag_set, LZ4F_ERROR_allocation_failed,
    LZ4F_ERROR_srcSize_tooLarge, LZ4F_ERROR_dstMaxSize_tooSmall, LZ4F_ERROR_frameHeader_incomplete,
    LZ4F_ERROR_frameType_unknown, LZ4F_ERROR_frameSize_wrong, LZ4F_ERROR_srcPtr_wrong,
    LZ4F_ERROR_decompressionFailed, LZ4F_ERROR_headerChecksum_invalid, LZ4F_ERROR_contentChecksum_invalid,
    LZ4F_ERROR_frameDecoding_alreadyStarted, LZ4F_ERROR_maxCode
} LZ4F_errorCodes;

/* replaces LZ4F_isError / LZ4F_getErrorName -- Conduit.hsc:149-153 (unsafe FFI call: never blocks) */
LZ4F_MI355X_API unsigned    LZ4F_isError(LZ4F_errorCode_t code);
LZ4F_MI355X_API const char* LZ4F_getErrorName(LZ4F_errorCode_t code);
LZ4F_MI355X_API unsigned    LZ4F_getVersion(void);

/* replaces LZ4F_createCompressionContext -- Conduit.hsc:199, :242 */
LZ4F_MI355X_API LZ4F_errorCode_t LZ4F_createCompressionContext(LZ4F_cctx** cctxPtr, unsigned version);
/* replaces LZ4F_freeCompressionContext -- Conduit.hsc:181, :210 (NULL is accepted) */
LZ4F_MI355X_API LZ4F_errorCode_t LZ4F_freeCompressionContext(LZ4F_cctx* cctx);
/* replaces LZ4F_compressBegin -- Conduit.hsc:292 */
LZ4F_MI355X_API size_t LZ4F_compressBegin(LZ4F_cctx* cctx, void* dstBuffer, size_t dstCapacity, const LZ4F_preferences_t* prefsPtr);
/* replaces LZ4F_compressBound -- Conduit.hsc:302 */
LZ4F_MI355X_API size_t LZ4F_compressBound(size_t srcSize, const LZ4F_preferences_t* prefsPtr);
/* replaces LZ4F_compressUpdate -- Conduit.hsc:311 (cOptPtr is always NULL there) */
LZ4F_MI355X_API size_t LZ4F_compressUpdate(LZ4F_cctx* cctx, void* dstBuffer, size_t dstCapacity,
                                           const void* srcBuffer, size_t srcSize, const LZ4F_compressOptions_t* cOptPtr);
/* LZ4F_flush: not bound by the reference; LZ4F_compressEnd is defined in terms of it */
LZ4F_MI355X_API size_t LZ4F_flush(LZ4F_cctx* cctx, void* dstBuffer, size_t dstCapacity, const LZ4F_compressOptions_t* cOptPtr);
/* replaces LZ4F_compressEnd -- Conduit.hsc:321 */
LZ4F_MI355X_API size_t LZ4F_compressEnd(LZ4F_cctx* cctx, void* dstBuffer, size_t dstCapacity, const LZ4F_compressOptions_t* cOptPtr);

/* replaces LZ4F_createDecompressionContext -- Conduit.hsc:568 */
LZ4F_MI355X_API LZ4F_errorCode_t LZ4F_createDecompressionContext(LZ4F_dctx** dctxPtr, unsigned version);
/* replaces LZ4F_freeDecompressionContext -- Conduit.hsc:545 (NULL is accepted) */
LZ4F_MI355X_API LZ4F_errorCode_t LZ4F_freeDecompressionContext(LZ4F_dctx* dctx);
LZ4F_MI355X_API void   LZ4F_resetDecompressionContext(LZ4F_dctx* dctx);
LZ4F_MI355X_API size_t LZ4F_headerSize(const void* src, size_t srcSize);
/* replaces LZ4F_getFrameInfo -- Conduit.hsc:579 */
LZ4F_MI355X_API size_t LZ4F_getFrameInfo(LZ4F_dctx* dctx, LZ4F_frameInfo_t* frameInfoPtr, const void* srcBuffer, size_t* srcSizePtr);
/* replaces LZ4F_decompress -- Conduit.hsc:591 (dOptPtr is always NULL there) */
LZ4F_MI355X_API size_t LZ4F_decompress(LZ4F_dctx* dctx, void* dstBuffer, size_t* dstSizePtr,
                                       const void* srcBuffer, size_t* srcSizePtr, const LZ4F_decompressOptions_t* dOptPtr);

/* the same twelve (+3) under a private prefix, for processes that also map liblz4 */
LZ4F_MI355X_API unsigned    lz4f_mi355x_isError(size_t code);
LZ4F_MI355X_API const char* lz4f_mi355x_getErrorName(size_t code);
LZ4F_MI355X_API size_t lz4f_mi355x_createCompressionContext(LZ4F_cctx** cctxPtr, unsigned version);
LZ4F_MI355X_API size_t lz4f_mi355x_freeCompressionContext(LZ4F_cctx* cctx);
LZ4F_MI355X_API size_t lz4f_mi355x_compressBegin(LZ4F_cctx* cctx, void* dst, size_t cap, const LZ4F_preferences_t* prefs);
LZ4F_MI355X_API size_t lz4f_mi355x_compressBound(size_t srcSize, const LZ4F_preferences_t* prefs);
LZ4F_MI355X_API size_t lz4f_mi355x_compressUpdate(LZ4F_cctx* cctx, void* dst, size_t cap, const void* src, size_t n, const LZ4F_compressOptions_t* o);
LZ4F_MI355X_API size_t lz4f_mi355x_flush(LZ4F_cctx* cctx, void* dst, size_t cap, const LZ4F_compressOptions_t* o);
LZ4F_MI355X_API size_t lz4f_mi355x_compressEnd(LZ4F_cctx* cctx, void* dst, size_t cap, const LZ4F_compressOptions_t* o);
LZ4F_MI355X_API size_t lz4f_mi355x_createDecompressionContext(LZ4F_dctx** dctxPtr, unsigned version);
LZ4F_MI355X_API size_t lz4f_mi355x_freeDecompressionContext(LZ4F_dctx* dctx);
LZ4F_MI355X_API size_t lz4f_mi355x_getFrameInfo(LZ4F_dctx* dctx, LZ4F_frameInfo_t* fi, const void* src, size_t* srcSize);
LZ4F_MI355X_API size_t lz4f_mi355x_decompress(LZ4F_dctx* dctx, void* dst, size_t* dstSize, const void* src, size_t* srcSize, const LZ4F_decompressOptions_t* o);

/* The two finalizers the reference defines verbatim in C (Conduit.hsc:163-189, :539-553) and
 * takes the address of (Conduit.hsc:191, :555); shipped here so a binding that does not use
 * inline-c still finds them. */
LZ4F_MI355X_API void haskell_lz4_freeCompressionContext(LZ4F_cctx** ctxPtr);
LZ4F_MI355X_API void haskell_lz4_freeDecompressionContext(LZ4F_dctx** ctxPtr);

/* ------------------------------------------------------------------------------------------
 * PART 2 -- bulk extension (new; what the batched conduits call).  All functions return an
 * LZ4F-style size_t (test with LZ4F_isError).
 * ------------------------------------------------------------------------------------------ */

/* why the last failing call on this thread failed (HIP error text etc.); never NULL */
LZ4F_MI355X_API const char* lz4f_mi355x_last_error(void);
/* number of usable HIP devices (0 when there is none: every compute entry then fails loudly) */
LZ4F_MI355X_API int lz4f_mi355x_device_count(void);
/* which device the calling thread's contexts and engines are created on (default: 0, or the
 * LZ4F_MI355X_DEVICE environment variable) */
LZ4F_MI355X_API size_t lz4f_mi355x_set_device(int device);
/* The host-pointer entry points (the twelve LZ4F_* functions, compressFrame / decompressFrame, the conduits) borrow an engine
 * - a HIP stream, pinned staging, device workspace - from a process-wide pool for the duration of a call and give it back;
 * nothing is owned by a thread.  This frees the engines that are idle right now (the pool refills on demand). */
LZ4F_MI355X_API void lz4f_mi355x_release_engines(void);

/* Worst-case size of a whole frame for srcSize bytes (header + blocks + EndMark + checksum). */
LZ4F_MI355X_API size_t lz4f_mi355x_compressFrameBound(size_t srcSize, const LZ4F_preferences_t* prefs);

/* Host-pointer bulk calls: one complete frame per call.  The frame's blocks go to the GPU in slabs of consecutive blocks (64 MiB),
 * several slabs in flight - two engines per device, each on a host thread of its own - so that uploads, kernels and downloads
 * overlap; page-locked buffers (lz4f_mi355x_host_alloc) are read and written by the DMA engines directly, pageable ones through
 * pinned staging.  compressFrame == the bytes the streaming API would produce for the same input fed in whole blocks (up to the
 * match finder's choice of matches, which is not deterministic). */
LZ4F_MI355X_API size_t lz4f_mi355x_compressFrame(void* dst, size_t dstCapacity, const void* src, size_t srcSize,
                                                 const LZ4F_preferences_t* prefs);
/* BLOCK LIST of a finished frame held in host memory - a frame of this library's host paths (compressFrame, the LZ4F_* streaming
 * calls, the conduits) or of any other LZ4 encoder (an archive made by liblz4 years ago).  appendBlockList walks the frame's size words
 * once on the host (a 4-byte read per block, no GPU) and writes, at buf + frameSize, the skippable frame lz4f_mi355x_dev_decompressFrame
 * looks for at a stream's end: where every block's size word is.  The device decoder then checks those positions link by link in parallel
 * instead of walking them - a walk is one dependent read per block, 0.12 ms for 256 blocks of 4 MiB and 10x that for 64 KiB blocks - and
 * every other LZ4 reader skips the extra frame as the format says.  frameSize must be exactly the frame (header .. EndMark / content
 * checksum); returns frameSize + the bytes added (nothing is added to a frame without blocks), or an error code
 * (dstMaxSize_tooSmall: capacity; frameSize_wrong: the frame does not end at frameSize).  blockListSize: the bytes appendBlockList would add.
 * The frame must start 16-byte aligned in DEVICE memory when it is decoded for the list to be looked at (it is a hint: without it the
 * walk happens as before). */
LZ4F_MI355X_API size_t lz4f_mi355x_blockListSize(const void* frame, size_t frameSize);
LZ4F_MI355X_API size_t lz4f_mi355x_appendBlockList(void* buf, size_t frameSize, size_t capacity);
/* Decodes the first frame found in src. *srcConsumed (optional) = bytes of src used. */
LZ4F_MI355X_API size_t lz4f_mi355x_decompressFrame(void* dst, size_t dstCapacity, const void* src, size_t srcSize,
                                                   size_t* srcConsumed);
/* The same without an output buffer of the caller's: `yield` gets the decoded bytes slab by slab, in order, on the calling
 * thread (each slab is valid during the call only).  Memory is bounded by the slabs in flight whatever the frame claims.
 * Returns the decoded size. */
typedef void (*lz4f_mi355x_yield_fn)(void* user, const void* data, size_t size);
LZ4F_MI355X_API size_t lz4f_mi355x_decompressFrameTo(lz4f_mi355x_yield_fn yield, void* user, const void* src, size_t srcSize,
                                                     size_t* srcConsumed);
/* A frame decoded BATCH BY BATCH, for callers that receive a stream and must not hold all of it (the bounded decompressBatched conduit;
 * the reference's `decompress` holds one max(hint, 16 KiB) buffer, Conduit.hsc:634-659).  The caller walks the size words over what arrives:
 *   fdec_create   parses a complete frame header (LZ4F_headerSize says how many bytes that is); returns its size, fills *info (may be NULL)
 *   fdec_blocks   a run of WHOLE blocks - [u32 size word | payload | u32 checksum if the header says so]* - is decoded through the bulk path
 *                 (slabs of blocks in flight over the devices lz4f_mi355x_use_devices named) and handed to `yield` in order; returns the decoded
 *                 bytes.  Linked frames: the last 64 KiB handed over are kept inside for the next run.  Memory: the run + the slabs in flight.
 *   fdec_end      `tail` = the EndMark and, if the header asks for one, the content checksum behind it: verifies contentSize and the checksum
 *                 over everything the runs produced; returns the bytes of tail consumed (4 or 8)
 *   fdec_free     always, also after an error */
typedef struct lz4f_mi355x_fdec lz4f_mi355x_fdec;
LZ4F_MI355X_API size_t lz4f_mi355x_fdec_create(lz4f_mi355x_fdec** out, const void* header, size_t headerBytes, LZ4F_frameInfo_t* info);
LZ4F_MI355X_API size_t lz4f_mi355x_fdec_blocks(lz4f_mi355x_fdec* d, lz4f_mi355x_yield_fn yield, void* user, const void* blocks, size_t blocksBytes);
LZ4F_MI355X_API size_t lz4f_mi355x_fdec_end(lz4f_mi355x_fdec* d, const void* tail, size_t tailBytes);
LZ4F_MI355X_API void   lz4f_mi355x_fdec_free(lz4f_mi355x_fdec* d);

/* How many GPUs the bulk calls above deal their slabs over (round-robin, starting at the calling thread's device; default 1).
 * Blocks of an independent-block frame need nothing from each other: no collective, the host puts the slabs' output in order.
 * Process-wide.  count must be <= the visible devices (test switch: with LZ4F_MI355X_LOGICAL_DEVICES=n in the environment up to
 * n "logical" devices are accepted and mapped onto the visible ones, d mod visible - the dealing code runs as on n GPUs). */
LZ4F_MI355X_API size_t lz4f_mi355x_use_devices(int count);
/* Page-locked host memory for the bulk calls' src / dst (what the batched conduits gather their chunks in). */
LZ4F_MI355X_API void*  lz4f_mi355x_host_alloc(size_t size);
LZ4F_MI355X_API void   lz4f_mi355x_host_free(void* p);

/* ---- device-resident engine: everything stays in HBM, nothing synchronises with the host ---- */
typedef struct lz4f_mi355x_engine lz4f_mi355x_engine;

/* borrowStream == 0: the engine creates (and owns) a non-blocking stream on `device`; hipStream is ignored.
 * borrowStream != 0: all work is enqueued on the caller's hipStream_t `hipStream` (NULL = HIP's default stream). */
LZ4F_MI355X_API size_t lz4f_mi355x_engine_create(lz4f_mi355x_engine** out, int device, void* hipStream, int borrowStream);
LZ4F_MI355X_API size_t lz4f_mi355x_engine_free(lz4f_mi355x_engine* e);
LZ4F_MI355X_API void*  lz4f_mi355x_engine_stream(lz4f_mi355x_engine* e);

/* DETERMINISM.  liblz4 maps equal input to equal bytes.  This encoder, by default, does not: the sixteen waves of a workgroup search
 * neighbouring slices of a 64 KiB tile at once and share one hash table, so which earlier occurrence a position finds depends on
 * which wave got there first.  Every frame is a valid LZ4 frame that decodes to the input, and the size varies by ~1e-5 between
 * runs (4 GiB of the bench input: 2 189 936 735 .. 2 189 966 976 bytes) - but two compressions of the same input are in general
 * NOT byte-identical.  Where that matters (reproducible archives, deduplication, content-addressed stores) switch the engine to
 * the deterministic search (round 4: csrc/encode_solo.cuh): one wave per 64 KiB chunk with a hash table of its own - nothing shared
 * between waves, so the records are a function of the input alone; equal input then gives equal bytes, on the bench input at 1.4x
 * the default match finder's time and the same ratio (text: 6x the time, 2 % of the ratio; until round 4: one wave per workgroup of the shared search
 * parsing in order, 10x), with the worst-case record workspace, 2 bytes per input byte.  Engines of the host-pointer calls
 * and of the LZ4F_* streaming functions read LZ4F_MI355X_DETERMINISTIC=1 from the environment when they are made.
 * Decoding is deterministic always. */
LZ4F_MI355X_API size_t lz4f_mi355x_engine_set_deterministic(lz4f_mi355x_engine* e, int enable);

/* Optional per-kernel timing with HIP events recorded on the engine's stream around each kernel of the last
 * compress / decompress call.  get_timing synchronises the stream and fills ms[] (milliseconds):
 *   [0] find_matches  [1] layout  [2] emit  [3] xxh32 (compress)  [4] walk  [5] xxh32 (verify)  [6] decode (all kernels)
 *   [7] finish  [8] decode: parse kernel  [9] decode: copy kernel
 *   [10] the whole compress call  [11] the whole decompress call (first kernel's start to last kernel's end on the engine's stream:
 *        the block-checksum verification runs beside the decode kernels on a stream of the engine's own, so [5] + [6] > [11])
 * entries of kernels that did not run are 0.
 * get_timing_n fills the first min(n, LZ4F_MI355X_TIMING_SLOTS) slots of a float[n] - the call to use: the slot count has grown
 * (10 in rounds 1-2, 12 since round 3) and may grow again.  get_timing (no capacity argument) keeps its ORIGINAL contract and
 * writes exactly LZ4F_MI355X_TIMING_SLOTS_V1 = 10 floats, so a caller built against an older header is never overrun. */
#define LZ4F_MI355X_TIMING_SLOTS 12
#define LZ4F_MI355X_TIMING_SLOTS_V1 10
LZ4F_MI355X_API size_t lz4f_mi355x_engine_set_timing(lz4f_mi355x_engine* e, int enable);
LZ4F_MI355X_API size_t lz4f_mi355x_engine_get_timing(lz4f_mi355x_engine* e, float* ms);
LZ4F_MI355X_API size_t lz4f_mi355x_engine_get_timing_n(lz4f_mi355x_engine* e, float* ms, size_t n);

/* result record the device writes; read it back after synchronising the stream */
typedef struct {
    uint64_t size;        /* compress: frame bytes written; decompress: decoded bytes */
    uint64_t consumed;    /* decompress: frame bytes consumed (incl. EndMark / checksum) */
    uint32_t status;      /* LZ4F_errorCodes value, 0 = ok */
    uint32_t n_blocks;
    uint32_t first_bad_block;
    uint32_t flags;       /* decoded FLG byte (decompress) */
} lz4f_mi355x_result;

/* WHICH FLAW DECIDES.  A frame with more than one flaw gets the verdict of the first of them in this order, from every one-shot
 * call - lz4f_mi355x_decompressFrame, lz4f_mi355x_dev_decompressFrame under every switch, lz4f_mi355x_dev_decompressBlocks and the
 * batch calls lz4f_mi355x_dev_decompressFrames[_usingDict / _usingDictSet] (tests/flaw_pairs.py: one_shot_verdict is this paragraph
 * in Python; tests/test_gpu_flaw_pairs.py holds the calls to it on frames with two flaws):
 *   1. the span and the offsets (batch calls: ERROR_srcPtr_wrong, ERROR_dstMaxSize_tooSmall);
 *   2. the header;
 *   3. the walk over ALL the size words, before any block is looked at: per block in frame order a size word above maxBlockSize
 *      (ERROR_maxBlockSize_invalid), a span that ends inside the word, the payload or the block checksum
 *      (ERROR_frameHeader_incomplete), and - device-pointer calls, linked frames too - a block whose provisional place,
 *      b * maxBlockSize, lies outside the window (ERROR_dstMaxSize_tooSmall); behind the EndMark the content checksum's word
 *      (ERROR_frameHeader_incomplete).  first_bad_block stays 0xFFFFFFFF.  So a bad size word or a truncation ANYWHERE in the frame
 *      beats a block that does not decode in front of it - where liblz4, which meets the blocks one by one, names that block;
 *   4. the blocks in order, in each block its checksum (ERROR_blockChecksum_invalid) before its decode (ERROR_GENERIC; or
 *      ERROR_dstMaxSize_tooSmall where the block decodes but not into the room the window leaves it): first_bad_block is that
 *      block - the first one, with one stated exception: for a malformed LINKED frame lz4f_mi355x_dev_decompressFrame and
 *      lz4f_mi355x_dev_decompressBlocks may name a later block of the same frame, with the same status (the batch calls name
 *      the first).  lz4f_mi355x_decompressFrame puts the blocks back to back and wants each to fit what is left of dst;
 *      lz4f_mi355x_dev_decompressBlocks has no level 3, 5 or 6: the table is the caller's;
 *   5. the content size (ERROR_frameSize_wrong);
 *   6. the content checksum (ERROR_contentChecksum_invalid).
 * lz4f_mi355x_dev_measureFrames keeps the same order over what it looks at (no checksum, no window).  The LZ4F_* streaming calls of
 * PART 1 and the conduits are drop-ins and have no order of their own: their answer is liblz4's, which is "the first flaw a
 * sequential reader meets" (tests/golden/flaw_pairs.json records it). */

/* Block table entry: where block i lives in the frame and in the output. */
typedef struct {
    uint64_t src_off;     /* offset of the payload (after the 4-byte size word) in the frame */
    uint64_t dst_off;     /* offset of the decoded block in the output */
    uint32_t word;        /* the size word as stored: bit31 = stored raw, bits 30..0 = payload bytes */
    uint32_t dst_size;    /* decoded bytes (filled by decode; blockSize-capacity on input) */
} lz4f_mi355x_block;

/* ALIGNMENT of the device pointers of every lz4f_mi355x_dev_* call below (tests/test_gpu_alignment.py moves each of them):
 *   - data buffers - d_src, d_dst, d_frame, the d_src / d_dst of the batch call and every span and window inside them - take ANY
 *     byte address: a frame inside a bigger receive buffer, a view that starts at byte 1.  The bytes written (deterministic
 *     encoders: the frame's bytes; every decoder: the output) and every verdict are the same at every address.
 *   - block tables (d_table, lz4f_mi355x_block: 64-bit words) and the batch call's d_src_off / d_dst_off: 8 bytes.
 *   - sequence indexes (d_index, 16-byte units): 16 bytes.
 *   - result records (d_result / d_results): 8 bytes.
 *   - the in-band call (indexCapacity == LZ4F_MI355X_INBAND): d_dst 16 bytes - the one requirement on a data buffer, checked:
 *     the call returns ERROR_GENERIC ("in-band index: the frame buffer must be 16-byte aligned") and writes nothing.
 *   - one DECISION depends on an address: lz4f_mi355x_dev_decompressFrame looks at a trailer (in-band index, block list) only when
 *     d_frame is 16-byte aligned; elsewhere the same stream is walked and parsed as a frame without one - same bytes, same
 *     size and consumed, other path bits (a hint, as said at lz4f_mi355x_appendBlockList).
 * Nothing is written outside [d_dst, d_dst + dstCapacity), the table's srcSize / blockSize + 1 entries, the index's capacity and the records.
 * Reads: the kernels bound every fetch from a frame by frameCapacity (the 16-byte fetches at a frame's end go byte by byte);
 * the block decoder's scalar fetches round a payload's start down and its end up to 4 bytes of ADDRESS, which are bytes of the
 * same frame (a size word in front, a checksum or the next size word / EndMark behind).  No read outside the extents a call
 * names is known; the tests do not probe for one at an allocation's edge. */

/* Bytes of device workspace the engine will hold for inputs up to srcSize (informational). */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_workspace_size(size_t srcSize, const LZ4F_preferences_t* prefs);

/* d_src[0..srcSize) -> one LZ4 frame at d_dst (device pointers).  Asynchronous on the engine's
 * stream.  d_result (device, optional) receives size/status; d_table (device, optional,
 * >= srcSize/blockSize+1 entries) receives the block table, which dev_decompressBlocks accepts
 * back to skip the serial walk over the size words.
 * Content checksum (prefs->frameInfo.contentChecksumFlag): XXH32 over the whole input is one
 * dependent chain, so ONE wave computes it (k_xxh32_content: the four accumulators as four
 * lanes) at ~1.4 GB/s - far below the codec; the word lands behind the EndMark as liblz4's does.  */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_compressFrame(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity,
                                                     const void* d_src, size_t srcSize, const LZ4F_preferences_t* prefs,
                                                     lz4f_mi355x_result* d_result, lz4f_mi355x_block* d_table);

/* First frame at d_frame[0..frameCapacity) -> d_dst.  Peeks the 7..19 header bytes (one small
 * device->host copy), then everything is asynchronous: a walk kernel chases the size words, block
 * checksums are verified on the GPU, blocks are decoded.  A content checksum present in the
 * frame is verified behind the decode (same single wave as above; a mismatch gives
 * ERROR_contentChecksum_invalid in result.status); an engine made with
 * LZ4F_MI355X_NO_CONTENT_CHECK set in the environment skips that, as liblz4 >= 1.9.4 can
 * (LZ4F_decompressOptions_t.skipChecksums).                                                   */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_decompressFrame(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity,
                                                       const void* d_frame, size_t frameCapacity,
                                                       lz4f_mi355x_result* d_result);

/* Table-driven variant: the caller already has the block table (from dev_compressFrame, or from
 * walking the size words on the host), so there is no walk and no host synchronisation at all.
 * `info` carries blockSizeID / blockMode / blockChecksumFlag of the frame.                     */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_decompressBlocks(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity,
                                                        const void* d_frame, size_t frameCapacity,
                                                        const lz4f_mi355x_block* d_table, uint32_t n_blocks,
                                                        const LZ4F_frameInfo_t* info, lz4f_mi355x_result* d_result);

/* Sequence index (optional side channel between this library's own compress and decompress; the frame itself stays a
 * plain LZ4 frame and decodes without it).  While it writes a block's payload the compressor notes, every 16 sequences,
 * where the token sits in the payload and which output position the sequence starts at; with that table the decoder
 * parses every 16 sequences on their own lane, finds the matches whose bytes sit in the payload itself, and copies in
 * parallel instead of walking one dependent chain per 4 MiB block (replaces the same inner loop of LZ4F_decompress,
 * Conduit.hsc:591).  The decoder still parses the payload itself -- the index only says where it may start -- and checks
 * that the pieces join up: a missing, stale or foreign index makes it fall back to the generic decoder, it cannot change
 * the bytes that come out.  Independent blocks only.  A stream with more sequences than the index has room for (about one
 * per 64 input bytes at the recommended size) gets an index marked unusable. */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_index_size(size_t srcSize, const LZ4F_preferences_t* prefs);       /* recommended bytes for d_index */
/* IN-BAND: with d_index == NULL and indexCapacity == LZ4F_MI355X_INBAND (d_table and d_result may then be NULL too) the index
 * and the list of the blocks' positions travel in the byte stream itself, as a skippable frame (magic 0x184D2A5E) right behind
 * the LZ4 frame: result.size includes it, d_dst must be 16-byte aligned and hold compressFrameBound + trailer_bound bytes.
 * liblz4, the `lz4` tool and the reference's `decompress` (Conduit.hsc:598: it stops at the EndMark) decode such a stream to the
 * same bytes; lz4f_mi355x_dev_decompressFrame finds the trailer from the stream's last 32 bytes and, after checking it against
 * the frame itself, skips the walk over the size words and parses with the index. */
#define LZ4F_MI355X_INBAND ((size_t)-1)
/* result.flags: bits 0..7 the frame's FLG byte, bit 8 a skippable frame was skipped; bits 12.. say which way a decompress call
 * went - a pure function of the call's arguments, the frame's header and trailer and the switches the engine was made with,
 * never of earlier calls (tests/test_gpu_parity.py: test_decode_path_by_input_class).  TRAILER and PARALLEL_WALK say which list
 * walk was PLANNED; whether its list was the chain of the frame's own size words, and so became the table, is WALK_DELIVERED
 * (tests/test_gpu_walks.py) */
#define LZ4F_MI355X_PATH_TABLE_GIVEN   0x001u   /* the caller's block table: no walk */
#define LZ4F_MI355X_PATH_TRAILER       0x002u   /* the size words' positions came from the frame's trailer (checked link by link) */
#define LZ4F_MI355X_PATH_PARALLEL_WALK 0x004u   /* the size words were looked for in parallel (small blocks) */
#define LZ4F_MI355X_PATH_INDEXED       0x008u   /* sequence index: parse per entry, direct matches, copier workgroups */
#define LZ4F_MI355X_PATH_SELF_INDEX    0x010u   /* linked frame without an index: the decoder made one */
#define LZ4F_MI355X_PATH_DOUBLING      0x020u   /* dense frame: pointer doubling was set up (the device decides whether it runs) */
#define LZ4F_MI355X_PATH_TRACE_HOPS    0x040u   /* dense frame: the hop-by-hop tracer was set up */
#define LZ4F_MI355X_PATH_WINDOW        0x080u   /* linked frame: the single-workgroup window kernel was launched (it returns at once behind a successful indexed decode) */
#define LZ4F_MI355X_PATH_FUSED         0x100u   /* fused parse+copy workgroups were launched (alone, or as what the others fall back to) */
#define LZ4F_MI355X_PATH_WAVE_PER_BLOCK 0x200u  /* small independent blocks: a wave per block */
#define LZ4F_MI355X_PATH_WORKGROUP_PER_BLOCK 0x800u /* few big independent blocks that may be dense: a workgroup per block with the window in LDS was launched beside the fused ones (the payload's density decides on the device which of the two decodes) */
#define LZ4F_MI355X_PATH_INDEX_DROPPED 0x400u   /* set on the device: the indexed kernels refused the index, the generic ones decoded */
#define LZ4F_MI355X_PATH_WALK_DELIVERED 0x2000u /* set on the device: the block table and this record's walk came from a list that was accepted link by link (the trailer's, the parallel or the seeded walk's); clear with a caller's table, a serial walk, or a list that was declined and walked again serially */
/* compress calls, result.flags bit 9: the encoder's record workspace (sized for a sequence per 5.3 input bytes on average - dense text has
 * one per 6..8 - instead of the format's worst case of one per 4: lz4f_mi355x_dev_workspace_size) was used up, and the 64 KiB tiles that
 * found it empty went out as literals.  The frame is valid and decodes to the input, it is only bigger than it could be.
 * LZ4F_MI355X_RECS_PER_TILE (1..16385 records per 64 KiB of input, read when an engine is made; default 12288 = 1.5 bytes of workspace
 * per input byte, 16385 = worst case for every tile, 1024 = 0.13 bytes per byte for data known to be sparse in matches) sizes it. */
#define LZ4F_MI355X_ENC_POOL_SHORT     0x200u
LZ4F_MI355X_API size_t lz4f_mi355x_trailer_bound(size_t srcSize, const LZ4F_preferences_t* prefs);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_compressFrameIndexed(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize,
                                                            const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_result,
                                                            lz4f_mi355x_block* d_table, void* d_index, size_t indexCapacity);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_decompressBlocksIndexed(lz4f_mi355x_engine* e, void* d_dst, size_t dstCapacity, const void* d_frame,
                                                               size_t frameCapacity, const lz4f_mi355x_block* d_table, uint32_t n_blocks,
                                                               const LZ4F_frameInfo_t* info, const void* d_index, size_t indexSize,
                                                               lz4f_mi355x_result* d_result);

/* BATCH: n_frames independent frames in one call, with no host synchronisation and no device->host copy.
 * Frame i is the first frame in d_src[src_off[i] .. src_off[i+1]); its output window is d_dst[dst_off[i] .. dst_off[i+1]).
 * d_src_off / d_dst_off: n_frames + 1 uint64 each, DEVICE memory.  srcBytes / dstBytes: the extents of d_src / d_dst (host values:
 * they size the workspace and bound every span).  d_results: n_frames records, DEVICE memory.  Asynchronous on the engine's stream.
 *   - A frame in a batch decodes exactly as it would alone: d_results[i] and the bytes of window i are what
 *     lz4f_mi355x_dev_decompressFrame gives for that span and window (status, size, consumed, n_blocks, first_bad_block,
 *     flags & 0x1FF), with LZ4F_MI355X_PATH_BATCH as the path bits (flags >> 12).  One difference: for a malformed LINKED
 *     frame first_bad_block is the first block that does not decode in its own block's room (as liblz4 judges it); the single
 *     call's linked-frame kernels may name a later block of the same frame.  Where the single call rejects a header on
 *     the host and returns the error code, the batch writes that code to d_results[i].status.  A skippable frame at the
 *     start of a span is reported as the single call reports it (flag bit 8, consumed = the skippable frame); this library's
 *     in-band trailer behind a frame is not used, and not counted in consumed (as with the single call).
 *   - Frames are isolated: no kernel writes outside window i on behalf of frame i, whatever its bytes are, and a malformed
 *     frame changes no other frame's result or bytes.  The offsets are checked on the device: src_off[i] > src_off[i+1] or a
 *     span ending past srcBytes gives that frame ERROR_srcPtr_wrong, the same of the window against dstBytes
 *     ERROR_dstMaxSize_tooSmall; nothing is written for it.  Windows that overlap each other are the caller's race.
 *   - The call itself fails only on a null engine, a null pointer with n_frames > 0, or a failed allocation (of a workspace of
 *     80 bytes per frame + 40 bytes per (n_frames + dstBytes / 64 KiB + 1) block-table entries, grown as needed).
 *     n_frames == 0 is a no-op that returns 0.  Bytes in a failed frame's window are unspecified, as with the single call.
 * Independent blocks are decoded a wave per block across all frames; linked frames a wave per frame with the blocks in order;
 * content checksums a wave per frame, side by side.  (Every block of a frame has its provisional place, block b at b * maxBlockSize,
 * inside the window, so frames whose windows do not overlap always fit the block table; where overlapping windows overflow it, the
 * independent frames behind the overflow are decoded a wave per frame too, with the same results.)  A big
 * frame of many blocks gets none of the single call's parallel walks, indexed or workgroup-per-block decoders: send such
 * frames through lz4f_mi355x_dev_decompressFrame.  Trailers and sequence indexes are not used. */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_decompressFrames(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                        const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                        void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                        lz4f_mi355x_result* d_results);
/* The same with a SHARED DICTIONARY: one dictionary for the whole batch, as LZ4F_decompress_usingDict applies one to a frame.  The history
 * in front of a frame's output (linked blocks), or in front of every block (independent blocks), is the dictionary: a match offset is
 * valid if and only if 0 < offset <= bytes in front in that scope + dictSize, and a match may begin in the dictionary and run on into
 * the output (and into the bytes it writes itself).  Frames that liblz4 made with LZ4F_compressFrame_usingCDict /
 * LZ4F_compressBegin_usingCDict decode here with the same dictionary, and the frames of lz4f_mi355x_dev_compressFrames_usingDict.
 *   - d_dict: dictSize bytes of DEVICE memory at any byte address, read only; it must stay valid until the stream has run the call and
 *     must not overlap d_dst.  Only the last 64 KiB of a longer dictionary are used (the pointer is advanced on the host).
 *   - dictSize == 0 (d_dict may then be NULL) is lz4f_mi355x_dev_decompressFrames for the same arguments: the same bytes, the same records.
 *     d_dict == NULL with dictSize > 0 and n_frames > 0 is a call error, like the other null pointers.
 *   - The header's dictID is never interpreted and never checked (liblz4 does not check it either): matching IDs to dictionaries is the
 *     caller's job.  A frame decoded with the wrong dictionary decodes to wrong bytes, caught only by a content checksum.
 *   - Everything said above about the plain call holds: spans, windows, isolation, the offset checks (nothing is read outside
 *     [d_dict, d_dict + dictSize) on the dictionary's behalf: the offset is checked before any read), the record's fields,
 *     LZ4F_MI355X_PATH_BATCH, the workspace from the arguments alone, no host synchronisation, a launch count that does not depend on
 *     n_frames, any byte alignment.  With a dictionary every block, independent ones too, goes through the wave-per-block decoder
 *     that parses on the scalar unit.
 *   - lz4f_mi355x_dev_measureFrames never looks at offsets: "measure, then decode with the dictionary" works with it as it is.
 * Not covered: the single-frame device calls, the host-pointer and streaming LZ4F_* calls, the conduits. */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_decompressFrames_usingDict(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                                  const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                                  void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                                  lz4f_mi355x_result* d_results, const void* d_dict, size_t dictSize);
#define LZ4F_MI355X_PATH_BATCH 0x1000u   /* result.flags bits 12..: the frame went through the batch decoder (dev_decompressFrames), or was made by the batch encoder (dev_compressFrames) */

/* BATCH MEASURE: what n_frames frames decode to, and the windows lz4f_mi355x_dev_decompressFrames needs for them, without decoding:
 * "receive -> measure -> decode" on one stream, for frames whose headers declare no content size.  The conventions are the batch
 * decoder's: frame i is the first frame in d_src[src_off[i] .. src_off[i+1]); d_src_off: n_frames + 1 uint64, DEVICE memory, 8-byte
 * aligned; the data at any byte address; srcBytes the extent of d_src (a host value: it sizes the workspace and bounds every span);
 * d_results: n_frames records, DEVICE memory.  Asynchronous on the engine's stream, no host synchronisation, no device->host copy,
 * and a number of kernel launches that does not depend on n_frames.  Nothing is written except d_results, d_dst_off and the engine's
 * workspace: there is no output buffer.  Spans that overlap are legal (they are only read).
 *   - d_results[i]: size = the decoded bytes, counted from the block's tokens (not taken from the header); consumed, n_blocks and
 *     flags & 0x1FF exactly what lz4f_mi355x_dev_decompressFrames reports for a frame it accepts (a skippable frame first in the span:
 *     flag bit 8, size 0, consumed = that skippable frame); the path bits (flags >> 12) are LZ4F_MI355X_PATH_BATCH; first_bad_block
 *     0xFFFFFFFF unless a block is malformed.  A frame that fails has size 0 (ERROR_frameSize_wrong: the measured size), and consumed
 *     and n_blocks 0 when it fails before its blocks are looked at.
 *   - The verdict is the batch decoder's wherever that needs no decoded byte: the span and the offsets (src_off[i] > src_off[i+1] or
 *     a span ending past srcBytes: ERROR_srcPtr_wrong for that frame only), the header, the size words, truncation, the EndMark and
 *     the content checksum's word, ERROR_frameSize_wrong where a declared content size differs from the measured one, and the
 *     decoder's bound on a span's blocks (more than span bytes / 5 + 2 of them - only empty stored blocks, 4 bytes each, get there -
 *     is ERROR_dstMaxSize_tooSmall to the batch decoder in every window, and so it is here, with W = 0); and every rule
 *     of the block grammar that needs neither output bytes nor history, judged against room = maxBlockSize as liblz4 judges it: a
 *     length run past the payload, the last-sequence rules, a match that ends fewer than 5 bytes before room, match-length bytes
 *     reaching the payload's last 4 bytes, a block decoding past maxBlockSize, a compressed block with an empty payload; a stored
 *     block decodes to its size.  Such a block gives ERROR_GENERIC with first_bad_block = the first of them.
 *   - NOT LOOKED AT, by design: match offsets (0 < offset <= bytes in front, history included), block checksums and content
 *     checksums.  The two offset bytes of a match are stepped over and nothing is hashed.  A frame that measure accepts may still be
 *     rejected by the decode for one of these three reasons, and for no other.
 *   - d_dst_off (n_frames + 1 uint64, DEVICE memory, 8-byte aligned; may be NULL): the exclusive prefix sum of W[i], the total in
 *     d_dst_off[n_frames] - as it is, the d_dst_off of lz4f_mi355x_dev_decompressFrames for the same d_src / d_src_off, with any
 *     dstBytes >= the total.  W[i] is the smallest window that call accepts for frame i; 0 for a frame measure rejects or that has
 *     no blocks.  The batch decoder gives block b of a frame its provisional place at b * maxBlockSize and wants every place inside
 *     the window (k_bf_head), an independent block decoded at its place and a linked one behind its predecessors, each in what is
 *     left of the window up to maxBlockSize (k_bf_table, k_bf_serial), and judges a last block with less than a block of room
 *     against a whole block (k_bf_finish); so, with n blocks of maxBlockSize bs and the last one decoding to g bytes,
 *         independent blocks: W = (n - 1) * bs + max(g, 1)        linked blocks: W = max(size, (n - 1) * bs + 1).
 *     W == size whenever every block but the last decodes to bs and the last one to at least a byte - the usual case; a frame
 *     written with flushes (short inner blocks) needs W > size; W <= n * bs always.
 *   - Workspace, from the call's arguments alone: 76 bytes per frame and 24 bytes per (n_frames + srcBytes / 256 + 1) block-table
 *     entries - under 0.1 byte per source byte - grown as needed.  A block needs only 5 bytes of source, so frames of many tiny
 *     blocks can overflow the table: the frames behind the overflow are measured a wave per frame, in order, with identical results.
 *   - The call itself fails only on a null engine, a null pointer with n_frames > 0 (d_dst_off excepted), or a failed allocation.
 *     n_frames == 0 returns 0 and enqueues nothing.
 * Every block of every frame, linked ones included (a size needs no history), is measured by a wave of its own.
 * Frames made with a dictionary measure like any other (offsets are not looked at): measure, then decode the same spans with
 * lz4f_mi355x_dev_decompressFrames_usingDict and the d_dst_off this call wrote. */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_measureFrames(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                     const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                     uint64_t* d_dst_off, lz4f_mi355x_result* d_results);

/* BATCH ENCODE: n_frames inputs, one frame each, in one call - the mirror image of lz4f_mi355x_dev_decompressFrames, with its conventions,
 * so that the output of one is the input of the other without the data visiting the host.  No host synchronisation, no device->host
 * copy, and a number of kernel launches that does not depend on n_frames.
 * Input i is d_src[src_off[i] .. src_off[i+1]); frame i is written at d_dst + dst_off[i] and may use the window d_dst[dst_off[i] ..
 * dst_off[i+1]).  d_src_off / d_dst_off: n_frames + 1 uint64 each, DEVICE memory, 8-byte aligned.  srcBytes / dstBytes: the extents of
 * d_src / d_dst (host values: they size the workspace and bound every span and window).  The data buffers, spans and windows take any byte
 * address.  d_results: n_frames records, DEVICE memory.  Asynchronous on the engine's stream.
 * prefs (NULL = defaults) holds for the whole batch: blockSizeID, blockMode, blockChecksumFlag, contentChecksumFlag, dictID and
 * compressionLevel mean what they mean to lz4f_mi355x_dev_compressFrame.  frameInfo.contentSize != 0 means "every frame's header declares
 * its own input's length" (the value itself is ignored; an empty input's header declares none, as a contentSize of 0 means to the single call).
 *   - A frame in a batch is the frame it would be alone.  The batch always uses the deterministic match finders (levels <= 2 and 3-12),
 *     whatever lz4f_mi355x_engine_set_deterministic says: frame i's bytes are exactly what lz4f_mi355x_dev_compressFrame writes for input i
 *     alone on an engine in deterministic mode with the same preferences (contentSize = that input's length where the batch was asked for
 *     content sizes), and d_results[i] has that call's size (frame bytes), consumed (input bytes), status, n_blocks and FLG byte
 *     (flags & 0xFF); first_bad_block is 0xFFFFFFFF and the path bits (flags >> 12) are LZ4F_MI355X_PATH_BATCH.  The record workspace is
 *     sized for the worst case of every chunk: LZ4F_MI355X_ENC_POOL_SHORT never appears.
 *   - Frames are isolated: nothing is written outside window i on behalf of frame i, nothing beyond `size` bytes of it when the frame
 *     succeeds, and nothing at all when it does not.  A window smaller than the frame gives that frame ERROR_dstMaxSize_tooSmall (size 0)
 *     and leaves every other frame as it would have been; a window of lz4f_mi355x_compressFrameBound(length of input i, prefs) always
 *     suffices.  src_off[i] > src_off[i+1] or a span ending past srcBytes gives that frame ERROR_srcPtr_wrong; dst_off[i] > dst_off[i+1]
 *     or a window ending past dstBytes ERROR_dstMaxSize_tooSmall; nothing is written for such a frame.  Bytes inside a failed frame's
 *     window are unspecified.  Windows that overlap each other are the caller's race; spans that overlap are legal (they are only read).
 *   - The workspace comes from the call's arguments alone: 72 bytes per frame, 128 bytes per (n_frames + srcBytes / 64 KiB + 1) block /
 *     chunk entries, and 8 bytes per (srcBytes / 4 + one per entry) sequence records - 2 bytes per source byte, grown as needed.  Spans
 *     that do not overlap never need more.  Where overlapping spans do: entries are handed out in frame order, and the first frame
 *     that does not get its own, with every non-empty frame behind it, fails with ERROR_srcSize_tooLarge; the frames in front of it
 *     are what they would have been.
 *   - The call itself fails only on a null engine, a null pointer with n_frames > 0, an invalid blockSizeID in prefs
 *     (ERROR_maxBlockSize_invalid, as the single call), or a failed allocation.  n_frames == 0 returns 0 and enqueues nothing.  An empty
 *     input is a valid frame (header + EndMark, + the checksum of nothing when asked for).
 * The match finders run a wave (levels <= 2) or a workgroup (3-12) per 64 KiB chunk across all frames; layout and block checksums a
 * wave per block; header, size words, EndMark and content checksum a wave per frame.  No sequence index, no in-band trailer and no block
 * table come out of this call, and a big input of many blocks gets one wave for its frame-level passes: send it through
 * lz4f_mi355x_dev_compressFrame, which puts the shared finder on it. */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_compressFrames(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                      const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                      void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                      const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_results);

/* The same with a SHARED DICTIONARY (the batch's LZ4F_compressFrame_usingCDict): the match finder may reach into the dictionary as if
 * it lay in front of every input (linked blocks), or in front of every block (independent blocks).  Small records, which have next to
 * nothing in front of them to match against, are what this is for.  Frame i decodes to input i with the same dictionary, through
 * lz4f_mi355x_dev_decompressFrames_usingDict and through liblz4's LZ4F_decompress_usingDict.
 *   - d_dict / dictSize: as for lz4f_mi355x_dev_decompressFrames_usingDict - device memory at any byte address, read only, valid until
 *     the stream has run the call, not overlapping d_dst; the last 64 KiB of a longer one; a dictionary of fewer than 4 bytes changes
 *     nothing (as with LZ4_loadDict).  dictSize == 0 (d_dict may be NULL) is lz4f_mi355x_dev_compressFrames: the same bytes and records.
 *     d_dict == NULL with dictSize > 0 and n_frames > 0 is a call error.
 *   - prefs->frameInfo.dictID is written to the header as before and means nothing else to this library: it is not derived from the
 *     dictionary and not checked on decode.  Matching IDs to dictionaries is the caller's job.
 *   - compressionLevel 3-12 with dictSize > 0: the call returns ERROR_compressionLevel_invalid and enqueues nothing.  Levels <= 2
 *     take it.  (The hash-chain finder inserts 960 positions per barrier round through one wave: seeding a raw 64 KiB dictionary
 *     would put 69 such rounds in front of every record.  At those levels a dictionary comes prepared:
 *     lz4f_mi355x_dev_createCDictHC below.)
 *   - Frame i is a function of input i, the dictionary and prefs alone: the same bytes in a batch of one and in a batch of many.  A
 *     match is cut where the dictionary ends and the input begins (liblz4 may let one run across; the decoders take both).
 *   - Everything said above about the plain call holds: spans, windows, isolation, the record's fields, LZ4F_MI355X_PATH_BATCH, the
 *     workspace formula (the dictionary adds nothing to it), no host synchronisation, a launch count independent of n_frames.
 * Every 64 KiB chunk's wave seeds its hash table from the dictionary: a small record pays for up to 64 KiB of seeding.  A dictionary
 * that serves many calls is better prepared once: lz4f_mi355x_dev_createCDict / lz4f_mi355x_dev_compressFrames_usingCDict below. */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_compressFrames_usingDict(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                                const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                                void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                                const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_results,
                                                                const void* d_dict, size_t dictSize);

/* A PREPARED DICTIONARY (liblz4's LZ4F_CDict for the batch encoder): the dictionary digested once, reused by every frame of every call.
 * lz4f_mi355x_dev_createCDict copies the last min(dictSize, 64 KiB) bytes of d_dict (DEVICE memory at any byte address) into device
 * memory of its own and seeds the match finder's hash table from them once (11 520 bytes: 3840 x (u16 position + u8 tag)); a scope's
 * first chunk then copies that table where lz4f_mi355x_dev_compressFrames_usingDict reads the dictionary and seeds it again.
 *   - The copy and one kernel are enqueued on the engine's stream; nothing synchronises with the host beyond what the allocation itself
 *     does.  d_dict may be reused or freed once the stream has run the call.
 *   - dictSize == 0 (d_dict may be NULL) makes an empty CDict.  A dictionary of 1-3 bytes is kept (the decoder honours it), the finder
 *     ignores it.  A NULL e or out, or a NULL d_dict with dictSize > 0, is ERROR_GENERIC; a failed allocation
 *     ERROR_allocation_failed; *out is then NULL and nothing is leaked.
 *   - A CDict belongs to the engine that made it: it is used with that engine only (another one gets ERROR_GENERIC, "cdict belongs to
 *     another engine", and nothing is enqueued) and freed before that engine is.  It is never written after its creation: one CDict
 *     serves any number of calls.  lz4f_mi355x_dev_freeCDict waits for the engine's stream, then frees; NULL is accepted.
 *   - lz4f_mi355x_cdict_data: the owned copy, DEVICE memory, its length in *size (size may be NULL) - what to hand to
 *     lz4f_mi355x_dev_decompressFrames_usingDict.  NULL and 0 for a NULL or empty CDict.
 * lz4f_mi355x_dev_compressFrames_usingCDict is lz4f_mi355x_dev_compressFrames_usingDict with the CDict's copy for d_dict / dictSize:
 * every sentence above holds, and frame i and d_results[i] are byte for byte what that call writes for the same inputs, prefs and
 * dictionary bytes.  A NULL or empty cdict is lz4f_mi355x_dev_compressFrames (the same kernels, the same bytes); compressionLevel 3-12
 * with a non-empty one of lz4f_mi355x_dev_createCDict returns ERROR_compressionLevel_invalid and enqueues nothing: that CDict has no
 * digest for the hash-chain finder, and making one per call is what a prepared dictionary is there to avoid.
 *
 * lz4f_mi355x_dev_createCDictHC is lz4f_mi355x_dev_createCDict plus the hash-chain finder's digest: the CDict then serves every
 * compressionLevel.  Arguments, errors, ownership, engine affinity, lz4f_mi355x_cdict_data and lz4f_mi355x_dev_freeCDict are as above.
 *   - Still one device allocation - the digest above, the hash-chain digest, the copy - which grows by at most 147 456 bytes: the
 *     finder's head (16 KiB) and 2 bytes for each of the at most 65 536 chain slots, as they stand once the dictionary's positions
 *     have been inserted in order.  One more kernel (one workgroup) is enqueued on the engine's stream; nothing synchronises.
 *   - lz4f_mi355x_dev_compressFrames_usingCDict with compressionLevel >= 3 and such a CDict runs the hash-chain finder with the
 *     dictionary in front of every frame (linked) or block (independent): a scope's first chunk loads the digest where it would
 *     clear its tables.  Every other sentence of that call's contract holds: spans, windows, isolation, the record's fields,
 *     LZ4F_MI355X_PATH_BATCH, the workspace formula, a launch count independent of n_frames, any byte alignment; frame i is a
 *     function of input i, the dictionary bytes, prefs and the level alone (and of LZ4F_MI355X_HC_ATTEMPTS / LZ4F_MI355X_HC_LAZY
 *     where set).  A match is cut at the seam, as at levels <= 2.
 *   - At levels <= 2 it is the plain CDict: the same kernel, the same bytes.  Empty, or of 1-3 bytes, it gives at levels 3-12 the
 *     frames of lz4f_mi355x_dev_compressFrames at that level, byte for byte (the copy is kept for the decoder).
 * lz4f_mi355x_cdict_has_hc: 1 when the CDict was made by lz4f_mi355x_dev_createCDictHC, else 0 (NULL: 0). */
typedef struct lz4f_mi355x_cdict lz4f_mi355x_cdict;
LZ4F_MI355X_API size_t lz4f_mi355x_dev_createCDict(lz4f_mi355x_engine* e, lz4f_mi355x_cdict** out, const void* d_dict, size_t dictSize);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_createCDictHC(lz4f_mi355x_engine* e, lz4f_mi355x_cdict** out, const void* d_dict, size_t dictSize);
LZ4F_MI355X_API int    lz4f_mi355x_cdict_has_hc(const lz4f_mi355x_cdict* c);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_freeCDict(lz4f_mi355x_cdict* c);
LZ4F_MI355X_API const void* lz4f_mi355x_cdict_data(const lz4f_mi355x_cdict* c, size_t* size);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_compressFrames_usingCDict(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                                 const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                                 void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                                 const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_results,
                                                                 const lz4f_mi355x_cdict* cdict);

/* A SET OF DICTIONARIES for the batch calls: one chosen per frame, by a slot the caller gives or by the dictID in the frame's own
 * header.  A store has a dictionary per table, schema, tenant or message type, and a new version whenever one is retrained; with a set
 * a mixed batch is one call, and a receiver decodes packed frames (lz4f_mi355x_dev_packFrames / _splitFrames / _readPackDirectory) each
 * with the dictionary its header names, on one stream, with no header read back and no side channel:
 *   compressFrames_usingDictSet -> packFrames ... readPackDirectory -> measureFrames -> decompressFrames_usingDictSet(d_slot = NULL)
 *
 * THE SET (lz4f_mi355x_dev_createDictSet): n_dicts (<= 65 536) members, cdicts[k] with the ID dictIDs[k] (both HOST arrays, read
 * during the call only).  The members are CDicts of the same engine, BORROWED, not copied: they must outlive the set, and the set is
 * freed before the engine.  A member that is NULL or an empty CDict is a dictionary of no bytes.  A receiver that only decodes makes
 * its members with lz4f_mi355x_dev_createCDict: the decoder needs only the bytes.  The set owns one small device table (per member 32
 * bytes, and 8 for the lookup: the IDs sorted, searched by bisection), uploaded on the engine's stream during the call; it is never
 * written again, so one set serves any number of calls and is not consumed by them.
 *   - dictIDs must be pairwise distinct.  A duplicate, a NULL e / out / array with n_dicts > 0, more than 65 536 members, or a member
 *     of another engine returns ERROR_GENERIC; lz4f_mi355x_last_error says which, *out is NULL.  A failed allocation returns
 *     ERROR_allocation_failed.  n_dicts == 0 makes a valid empty set (the arrays may be NULL).
 *   - lz4f_mi355x_dev_freeDictSet waits for the engine's stream, then frees, like lz4f_mi355x_dev_freeCDict; NULL is accepted.
 *   - lz4f_mi355x_dictset_count: the number of members (NULL: 0).
 *
 * SLOTS.  d_slot: n_frames uint32 in DEVICE memory, 4-byte aligned, read on the device.  d_slot[i] is a member's index < count, or
 * LZ4F_MI355X_DICT_NONE: frame i has no dictionary.  Any other value, LZ4F_MI355X_DICT_UNKNOWN included, makes that frame - and only
 * that frame - fail: status ERROR_GENERIC, size, consumed and n_blocks 0, first_bad_block 0xFFFFFFFF, flags =
 * (LZ4F_MI355X_PATH_BATCH | LZ4F_MI355X_PATH_DICT_UNKNOWN) << 12 with the low 12 bits 0.  Nothing is written in its window and no
 * dictionary byte is read on its behalf; a slot is held to the set before it indexes the table, so a forged one never reads outside
 * it.  The verdicts in order - compress: the offset checks as in the plain call, then the slot; decode: the offset checks, then the
 * header's own errors (frameHeader_incomplete, frameType_unknown, a bad descriptor or header checksum, a skippable frame cut short),
 * then the slot.
 *
 * lz4f_mi355x_dev_compressFrames_usingDictSet: every sentence of the lz4f_mi355x_dev_compressFrames_usingCDict contract holds per
 * frame.  Frame i and d_results[i] are byte for byte what that call writes for input i alone, in a batch of one, with the member
 * d_slot[i] and prefs whose frameInfo.dictID is that member's ID (an ID of 0 writes no dictID field).  A LZ4F_MI355X_DICT_NONE frame
 * is lz4f_mi355x_dev_compressFrames' frame with prefs as given (prefs->frameInfo.dictID included); a NULL or empty member gives the
 * plain frame with that member's ID.
 *   - compressionLevel 3-12: a non-empty member that was not made by lz4f_mi355x_dev_createCDictHC fails the whole call,
 *     ERROR_compressionLevel_invalid, nothing enqueued.  (Membership is known on the host, slots are not: the rule is over all members.)
 *   - set == NULL, a set of another engine, or d_slot == NULL, with n_frames > 0, is a call error (ERROR_GENERIC).  n_frames == 0
 *     returns 0 and enqueues nothing.
 *   - Unchanged: the workspace formula (the slot lives in the frame's record), a launch count that depends neither on n_frames nor on
 *     n_dicts, any byte alignment of the data, isolation, no host synchronisation.
 *
 * lz4f_mi355x_dev_decompressFrames_usingDictSet: every sentence of the lz4f_mi355x_dev_decompressFrames_usingDict contract holds per
 * frame.  Frame i's record and window bytes are what that call gives for that span and window alone with the member's bytes
 * (lz4f_mi355x_cdict_data); with LZ4F_MI355X_DICT_NONE or an empty member they are what lz4f_mi355x_dev_decompressFrames gives.
 * With d_slot == NULL the slot comes from the frame's header: no dictID field, a skippable frame, or a header that does not parse (the
 * frame fails with its own error) -> LZ4F_MI355X_DICT_NONE; a field whose value is a member's ID (0 too, when a member has it) -> that
 * member; any other value -> the unknown-slot failure above.  A dictID is still never VERIFIED against the dictionary's bytes: a frame
 * decoded with the wrong member is caught only by a content checksum.  The workspace is the plain call's and 4 bytes per frame (the
 * resolved slots); the launch count is the plain call's.
 *
 * lz4f_mi355x_dev_resolveDictIDs: one launch, a thread per frame; writes to d_slot[i] exactly what the d_slot == NULL decode uses for
 * frame i, or LZ4F_MI355X_DICT_UNKNOWN for an ID the set does not have - to see, count or override the choice before decoding.  A span
 * that does not lie in d_src (the decode call gives that verdict) gives LZ4F_MI355X_DICT_NONE; nothing is read outside the spans.
 * Not covered: raw (unprepared) dictionaries as members; the single-frame, host-pointer and streaming calls. */
typedef struct lz4f_mi355x_dictset lz4f_mi355x_dictset;
#define LZ4F_MI355X_DICT_NONE    0xFFFFFFFFu   /* slot value: this frame has no dictionary */
#define LZ4F_MI355X_DICT_UNKNOWN 0xFFFFFFFEu   /* written by lz4f_mi355x_dev_resolveDictIDs: the header names an ID the set does not have */
#define LZ4F_MI355X_PATH_DICT_UNKNOWN 0x4000u  /* result.flags path bit (flags >> 12): the frame failed because its slot is no member of the set */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_createDictSet(lz4f_mi355x_engine* e, lz4f_mi355x_dictset** out, uint32_t n_dicts,
                                                     const lz4f_mi355x_cdict* const* cdicts, const uint32_t* dictIDs);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_freeDictSet(lz4f_mi355x_dictset* s);
LZ4F_MI355X_API uint32_t lz4f_mi355x_dictset_count(const lz4f_mi355x_dictset* s);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_resolveDictIDs(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                      const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                      const lz4f_mi355x_dictset* set, uint32_t* d_slot);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_compressFrames_usingDictSet(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                                   const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                                   void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                                   const LZ4F_preferences_t* prefs, lz4f_mi355x_result* d_results,
                                                                   const lz4f_mi355x_dictset* set, const uint32_t* d_slot);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_decompressFrames_usingDictSet(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                                     const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                                     void* d_dst, size_t dstBytes, const uint64_t* d_dst_off,
                                                                     lz4f_mi355x_result* d_results,
                                                                     const lz4f_mi355x_dictset* set, const uint32_t* d_slot /* NULL: by each header's dictID */);

/* BATCH PACK: the frames of a batch back to back in one contiguous stream - what is stored or sent - made on the device, on the same
 * stream, behind lz4f_mi355x_dev_compressFrames (or its _usingDict / _usingCDict forms), from that call's windows and records as they
 * are: "compress -> pack -> send" with no record read back, no host prefix sum and no copy per frame.  d_src / srcBytes / d_src_off
 * are the compress call's d_dst / dstBytes / d_dst_off, d_results its records.  Back-to-back LZ4 frames are a valid concatenated .lz4
 * stream: `lz4 -d` decodes the packed bytes to the inputs in order, with or without the directory.
 * Conventions as for the other batch calls: offsets (n_frames + 1 uint64) and records in DEVICE memory, 8-byte aligned; the data at
 * any byte address; srcBytes / dstBytes host values that bound every span; asynchronous on the engine's stream, no host
 * synchronisation, no device->host copy, two kernel launches whatever n_frames is; the workspace is one control block.
 *   - Pack never parses frame bytes: it copies what the records say.  Frame i is usable when d_results[i].status == 0,
 *     src_off[i] <= src_off[i+1] <= srcBytes and d_results[i].size <= src_off[i+1] - src_off[i].  L[i] is that size when the frame is
 *     usable and 0 otherwise: a frame the encoder failed keeps its slot as an empty span, slot i stays frame i, and the batch decoder
 *     gives the empty span ERROR_frameHeader_incomplete as it does today.
 *   - Output: D = lz4f_mi355x_packDirectorySize(n_frames) with LZ4F_MI355X_PACK_DIRECTORY in flags, 0 without; d_dst_off[0] = D,
 *     d_dst_off[i+1] = d_dst_off[i] + L[i]; frame i's L[i] bytes stand at d_dst + d_dst_off[i].  The first d_dst_off[n_frames] bytes
 *     of d_dst, with d_dst_off, are what lz4f_mi355x_dev_measureFrames, lz4f_mi355x_dev_decompressFrames and _usingDict take as d_src,
 *     srcBytes and d_src_off.  Nothing is written outside d_dst[0 .. d_dst_off[n_frames]), the n_frames + 1 offsets and the record;
 *     nothing is read outside d_src[src_off[i] .. src_off[i] + L[i]), the offsets and the records.  d_dst_off is an array of its
 *     own: not d_src_off, and not inside d_dst.
 *   - d_pack (DEVICE memory, may be NULL): size = d_dst_off[n_frames]; consumed = the sum of L; n_blocks = the frames with L[i] > 0;
 *     first_bad_block = the first i whose record says status 0 but is not usable (offsets or a size that lie; 0xFFFFFFFF: none - the
 *     pack succeeds all the same); flags = LZ4F_MI355X_PATH_BATCH; status 0, but
 *       ERROR_dstMaxSize_tooSmall when d_dst_off[n_frames] > dstBytes: no byte of d_dst is written; d_dst_off and size still say
 *         what was needed;
 *       ERROR_srcSize_tooLarge when the directory is asked for and some L[i] > 0xFFFFFFFF (a length the directory's u32 cannot say;
 *         likewise more than 0x3FFFFFFB frames, whose payload size it cannot say): nothing is written to d_dst.
 *     (Both at once: ERROR_dstMaxSize_tooSmall.)
 *   - THE DIRECTORY (LZ4F_MI355X_PACK_DIRECTORY): one skippable frame at the front of the stream, which every LZ4 reader steps over as
 *     the format requires, so that the one buffer is all a receiver needs: u32 magic 0x184D2A5D, u32 payloadBytes = 16 + 4 * n_frames,
 *     then the payload: u32 tag 0x44505A4C ("LZPD"), u32 n_frames, u64 framesBytes (the sum of L), u32 L[n_frames].  Little-endian, at
 *     any alignment.  D = 24 + 4 * n_frames.
 *   - The call itself fails only on a null engine, a null pointer with n_frames > 0 (d_pack excepted), a failed allocation, or a d_dst
 *     range [d_dst, d_dst + dstBytes) that overlaps [d_src, d_src + srcBytes): ERROR_GENERIC ("d_dst overlaps d_src"), checked on the
 *     host, nothing enqueued.  n_frames == 0 returns 0 and enqueues nothing.
 * The copy is dealt by OUTPUT bytes, LZ4F_MI355X_PACK_TILE of them to a workgroup at a time, so that 16 384 frames of 350 bytes and
 * three frames of 4 MiB load the machine alike.
 *
 * THE RECEIVING SIDE.  lz4f_mi355x_packDirectorySize: D for n_frames frames (host arithmetic).
 * lz4f_mi355x_peekPackDirectory reads the directory's fixed 24 bytes from HOST memory (a receiver has the head of a message on the
 * host, or copies 24 bytes itself) -> D, and *n_frames and *framesBytes (each may be NULL); ERROR_frameHeader_incomplete for fewer
 * than 24 bytes (or a NULL head), ERROR_frameType_unknown for another magic or tag, ERROR_frameSize_wrong where payloadBytes !=
 * 16 + 4 * n_frames.  The stream is then D + framesBytes bytes.
 * lz4f_mi355x_dev_readPackDirectory turns the directory of the stream in d_pack[0 .. packBytes) into d_src_off (n_frames + 1 uint64,
 * DEVICE memory) for the measure and decode calls, one launch on the engine's stream, every read bounded by packBytes.  It checks, in
 * this order: the fixed part as the peek does; the stored n_frames against the argument (ERROR_frameSize_wrong); packBytes >= D
 * (ERROR_frameHeader_incomplete); framesBytes == the sum of L (ERROR_frameSize_wrong); D + framesBytes <= packBytes
 * (ERROR_frameHeader_incomplete).  When it accepts: d_src_off[0] = D, then the running sums; d_result (DEVICE memory, may be NULL):
 * status 0, size = framesBytes, consumed = D + framesBytes, n_blocks = n_frames.  When it refuses: n_frames + 1 zeros - every span
 * empty, so a forged directory never hands a later call a span outside the buffer (the batch calls' own span checks stand behind it
 * in any case) - and d_result: that status, size, consumed and n_blocks 0.  flags = LZ4F_MI355X_PATH_BATCH, first_bad_block
 * 0xFFFFFFFF.  The call itself fails only on a null engine, a null d_pack or d_src_off with n_frames > 0, or a failed allocation;
 * n_frames == 0 returns 0 and enqueues nothing. */
#define LZ4F_MI355X_PACK_DIRECTORY 0x1u     /* flags: write the frame directory in front of the frames */
#define LZ4F_MI355X_PACK_TILE      16384u   /* informational: the copy kernel's output tile, for tests and tools */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_packFrames(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                  const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                  const lz4f_mi355x_result* d_results,
                                                  void* d_dst, size_t dstBytes, uint64_t* d_dst_off,
                                                  unsigned flags, lz4f_mi355x_result* d_pack);
LZ4F_MI355X_API size_t lz4f_mi355x_packDirectorySize(uint32_t n_frames);
LZ4F_MI355X_API size_t lz4f_mi355x_peekPackDirectory(const void* head, size_t headBytes, uint32_t* n_frames, uint64_t* framesBytes);
LZ4F_MI355X_API size_t lz4f_mi355x_dev_readPackDirectory(lz4f_mi355x_engine* e, uint32_t n_frames,
                                                         const void* d_pack, size_t packBytes, uint64_t* d_src_off,
                                                         lz4f_mi355x_result* d_result);

/* BATCH SPLIT: the frame boundaries of a concatenated LZ4 stream, found on the device - the d_src_off that the measure and decode
 * calls take, for a stream that came WITHOUT a directory: a packed stream whose sender wrote none, `cat a.lz4 b.lz4`, the output of
 * writers that emit a frame per chunk, a log that frames are appended to.  Conventions as for the other batch calls: d_src in DEVICE
 * memory at any byte address; d_src_off (max_frames + 1 uint64) in DEVICE memory, 8-byte aligned, not inside d_src; d_split (one
 * record, DEVICE memory) may be NULL; srcBytes and max_frames are host values; asynchronous on the engine's stream, no host
 * synchronisation, no device->host copy.  Nothing is written but the max_frames + 1 offsets, the record and the engine's workspace;
 * nothing is read outside d_src[0 .. srcBytes).
 *   - THE DEFINITION is the serial walk, whatever the stream's bytes are:
 *         pos = 0; n = 0; bytes = 0; skipped = false
 *         loop: if pos == srcBytes: status = 0, stop
 *               S[pos .. srcBytes) begins with a skippable frame (any of the 16 magics) that fits: pos += 8 + its size; skipped = true
 *               ... with an LZ4 frame whose header parses and whose size words walk to the EndMark (and the content checksum's
 *                   word): start[n] = pos; n += 1; bytes += its length; pos += its length
 *               anything else: status = what the batch decoder says of such a span, stop - ERROR_frameHeader_incomplete (a cut
 *                   anywhere in a frame), ERROR_frameType_unknown (no magic; the legacy format's magic too), ERROR_reservedFlag_set,
 *                   ERROR_headerVersion_wrong, ERROR_maxBlockSize_invalid (a header's block size ID, or a size word above the
 *                   frame's block size), ERROR_headerChecksum_invalid
 *     No payload is parsed and no checksum verified: those verdicts stay with the measure and decode calls.
 *   - Output, with m = min(n, max_frames): d_src_off[i] = start[i] for i < m; every later entry, d_src_off[max_frames] included, is
 *     start[max_frames] when n > max_frames and pos otherwise.  Span i < m so runs from frame i's first byte to the next frame's
 *     first byte: the skippable frames behind frame i (this library's in-band trailer among them) are inside it, and the batch decoder
 *     leaves them alone.  Skippable frames in front of the first frame (a pack directory) are in no span; surplus slots are empty
 *     spans, which the batch decoder gives ERROR_frameHeader_incomplete; the frame the walk stops at is not listed.  So
 *     (d_src, consumed, d_src_off, max_frames) are the d_src, srcBytes, d_src_off and n_frames of the measure and decode calls.
 *   - d_split: status = the walk's, or ERROR_dstMaxSize_tooSmall when the walk ended with 0 but n > max_frames (a grammar error
 *     wins); consumed = pos; n_blocks = n, ALL the frames found, so that the caller knows what to ask for; size = bytes, the frames'
 *     own; first_bad_block = n when the walk stopped on an error, else 0xFFFFFFFF; flags: bit 8 when a skippable frame was stepped
 *     over, and the path bits (flags >> 12): LZ4F_MI355X_PATH_BATCH | LZ4F_MI355X_PATH_PARALLEL_WALK when the parallel kernels
 *     delivered, LZ4F_MI355X_PATH_BATCH alone when the serial kernel did.
 *   - HOW: every byte position is looked at once (a streaming read); a position with an LZ4 magic and a header that parses, or a
 *     skippable magic whose frame fits, is a node, and position 0 is one.  A thread per node walks its size words to where its frame
 *     ends; the end is looked up in the node list; the true frames are the nodes REACHABLE from position 0, marked by pointer
 *     doubling - a .lz4 file inside a stored block or a skippable frame is a node that nothing points at.  The node list holds
 *         max_frames + srcBytes / LZ4F_MI355X_SPLIT_SHARE + 64   nodes (at most 0xFFFFFFF0),
 *     and the workspace is srcBytes / 8 bytes of position bits, 4 bytes per 16 KiB, and 33 bytes per node: from the two arguments
 *     alone, grown as needed.  A stream with more nodes (magics with valid headers packed into payloads) is walked by one thread
 *     instead, behind the parallel kernels, with the same answer.  Launches: 6 and ceil(log2(node list)) doubling rounds, never a
 *     function of the stream's bytes.
 *   - A frame of B blocks costs ONE thread B dependent reads, about 0.35 us each (MI355X, 176 MiB of stream: 0.15 ms as 4096 frames
 *     of 2 blocks, 0.32 ms as 8 frames of 512 blocks): this call is for streams of many frames, and does not replace the single
 *     call's parallel walks of one big frame.
 *   - The call itself fails only on a null engine, a null d_src or d_src_off with max_frames > 0, a failed allocation (or a stream
 *     beyond 2^45 bytes: ERROR_srcSize_tooLarge).  max_frames == 0 returns 0 and enqueues nothing.
 * LZ4F_MI355X_SPLIT_SERIAL set in the environment when the engine is made skips the parallel kernels (a test switch). */
#define LZ4F_MI355X_SPLIT_SHARE 256u        /* informational: stream bytes per spare node of the split's node list */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_splitFrames(lz4f_mi355x_engine* e,
                                                   const void* d_src, size_t srcBytes,
                                                   uint32_t max_frames, uint64_t* d_src_off,
                                                   lz4f_mi355x_result* d_split);
/* The same walk over a stream in HOST memory, by one host thread (no device is touched, no engine needed): src_off and split are host
 * memory, the answer is the device call's, the path bits are 0.  What a caller without the device call does after copying the stream
 * down - tools/batch_split.py times the device call against exactly that. */
LZ4F_MI355X_API size_t lz4f_mi355x_splitFrames(const void* src, size_t srcBytes, uint32_t max_frames, uint64_t* src_off,
                                               lz4f_mi355x_result* split);

/* BATCH TRAIN: a dictionary made from a batch of samples on the device - the one step of the dictionary's life that liblz4 leaves to
 * `zstd --train` on a host.  The samples are spans of one device buffer, as the inputs of lz4f_mi355x_dev_compressFrames are; the
 * result goes straight into lz4f_mi355x_dev_createCDict[HC] on the same stream.  Conventions as for the other batch calls: sample i is
 * d_src[src_off[i] .. src_off[i+1]); d_src and d_dict in DEVICE memory at any byte address; d_src_off (n_samples + 1 uint64) in DEVICE
 * memory, 8-byte aligned; d_result (one record, DEVICE memory) may be NULL; srcBytes and dictSize are host values; asynchronous on the
 * engine's stream, no host synchronisation, no device->host copy.  Spans that overlap are legal.  Nothing is written but
 * d_dict[0 .. dictSize), the record and the engine's workspace; nothing is read outside the valid spans and the offsets.
 *   - params (NULL: all defaults; a field that is 0: its default): k, the segment length in bytes, d <= k <= 4096
 *     (LZ4F_MI355X_TRAIN_K); d, the bytes hashed at a position, 4, 6 or 8 (LZ4F_MI355X_TRAIN_D); f, the bits of the hash,
 *     16 <= f <= 22 (LZ4F_MI355X_TRAIN_F); rounds, 1 <= rounds <= 64 (LZ4F_MI355X_TRAIN_ROUNDS); reserved stays 0.
 *   - THE DEFINITION.  The device's bytes are this sequential statement's, byte for byte:
 *     1. The corpus C is the valid samples back to back, in index order; N its length.  A span with src_off[i] > src_off[i+1] or an end
 *        past srcBytes contributes nothing.  A sample is taken only while the running total stays <= srcBytes: the first that does not
 *        fit, and all behind it, are dropped (only overlapping spans get there).  Dmers and segments may cross the samples' seams.
 *     2. M = N - d + 1 dmers (N < d: the dictionary is all zeros, used = 0, no round is run).  For j < M,
 *            h(j) = ((the d bytes at C[j] as a little-endian u64) * 0x9E3779B185EBCA87 mod 2^64) >> (64 - f)
 *        and freq[x] is the number of j with h(j) == x.
 *     3. m = min(k - d + 1, M) dmers make a window; the window starts are p in [0, W), W = M - m + 1.  prev(j) is the largest j' < j
 *        with h(j') == h(j), or -1.  score(p; F) = the sum of F[h(j)] over the j in [p, p + m) with prev(j) < p: F over the window's
 *        DISTINCT hashes.
 *     4. E = max(1, min(dictSize / k, W)) epochs; epoch e holds the starts [e * W / E, (e + 1) * W / E), by integer division.
 *     5. tail = dictSize.  For each of up to `rounds` rounds: S = a snapshot of freq; every epoch picks p_e, the lowest p of the epoch
 *        that maximises score(p; S); then, for e = 0 .. E - 1 in order: the epoch is skipped if score(p_e; S) == 0, and skipped as
 *        STALE if 2 * score(p_e; freq) < score(p_e; S) (it picks afresh in the next round); otherwise the window is trimmed to
 *        [s0, s1], its first and last j with freq[h(j)] > 0, the segment is C[s0 .. s1 + d), take = min(its length, tail), its
 *        first `take` bytes are copied to d_dict[tail - take .. tail), tail -= take, and freq[h(j)] = 0 for every j in [s0, s1];
 *        the commits stop when tail reaches 0.  The rounds end when tail == 0 or when a round appended nothing.
 *     Picking every segment in parallel against one snapshot would fill the dictionary with the same hot content once per epoch; the
 *     exact serial order needs a launch per segment.  Scores only fall as counts are zeroed, so the snapshot score bounds the live
 *     one from above: deferring the picks that lost half of theirs keeps the result within a few per cent of the serial order's.
 *   - Output: exactly dictSize bytes.  The trained content is right-aligned, d_dict[dictSize - used .. dictSize), the best segments
 *     last - where an encoder's offsets are shortest - and the front is zero-filled: (d_dict, dictSize) go into
 *     lz4f_mi355x_dev_createCDict[HC] as they are, no size read back.
 *   - d_result: size = used; consumed = N; n_blocks = the segments appended; first_bad_block = the first sample whose span is invalid
 *     (0xFFFFFFFF: none); status = 0; flags = LZ4F_MI355X_PATH_BATCH << 12, and in the low 8 bits the rounds that were run.
 *   - The workspace, from the arguments alone, grown as needed: 7 bytes per byte of srcBytes (the corpus, 4 bytes of hash and 2 of
 *     look-back per position), 8 per sample, 4 << f for the counts, 8 * max(1, dictSize / k) for the picks, and less than 1 KiB.
 *   - Launches: one fill, 4 to set up, and 2 * rounds - a function of `rounds` alone, never of n_samples, the bytes or dictSize / k;
 *     the kernels of a round that is no longer needed return at once.  No kernel waits on another workgroup.  The look-back costs up
 *     to k compares per position, once; a round is O(N), and its commit one workgroup's walk over the epochs.
 *   - The call itself fails, and enqueues nothing, on: a null engine; parameters out of range (ERROR_GENERIC, lz4f_mi355x_last_error
 *     names the field); dictSize > 65536 (ERROR_GENERIC: LZ4 never reads further back); srcBytes >= 2^31 (ERROR_srcSize_tooLarge);
 *     then, with n_samples > 0 and dictSize > 0, a null d_src, d_src_off or d_dict, or a failed allocation.  n_samples == 0 or
 *     dictSize == 0 returns 0 and enqueues nothing.
 *   - NOT COVERED: samples in host memory (copy them up: there is no host-pointer form); entropy tables (LZ4 has none: the dictionary
 *     is raw content); a dictID - the caller's to choose, in prefs.frameInfo.dictID or a dictionary set's. */
#define LZ4F_MI355X_TRAIN_K      64u        /* the defaults: segment bytes */
#define LZ4F_MI355X_TRAIN_D      8u         /*   bytes hashed at a position */
#define LZ4F_MI355X_TRAIN_F      18u        /*   bits of the hash */
#define LZ4F_MI355X_TRAIN_ROUNDS 16u        /*   rounds at most */
#define LZ4F_MI355X_TRAIN_TILE      4096u   /* informational: the corpus positions a workgroup of the training kernels takes at a time */
#define LZ4F_MI355X_TRAIN_SCAN_TILE 1024u   /* informational: the samples a step of the offsets' scan takes */
typedef struct { uint32_t k, d, f, rounds; uint32_t reserved[4]; } lz4f_mi355x_train_params;   /* 0 = default, each field */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_trainDict(lz4f_mi355x_engine* e, uint32_t n_samples,
                                                 const void* d_src, size_t srcBytes, const uint64_t* d_src_off,
                                                 void* d_dict, size_t dictSize,
                                                 const lz4f_mi355x_train_params* params /* NULL: defaults */,
                                                 lz4f_mi355x_result* d_result /* may be NULL */);

/* Per-block XXH32 of n_blocks byte ranges: d_out[i] = XXH32(d_base + off[i], len[i], 0) (row a5). */
LZ4F_MI355X_API size_t lz4f_mi355x_dev_xxh32(lz4f_mi355x_engine* e, const void* d_base, const uint64_t* d_off,
                                             const uint32_t* d_len, uint32_t n_blocks, uint32_t* d_out);

/* ---- C++ mirror of the reference's conduits, driven through callbacks (host side above the
 *      C ABI; see lz4_frame_conduit_amd/csrc/conduit.hpp).  `await` returns the next input chunk
 *      (size 0 at end of stream: sets *data = NULL); `yield` receives each output ByteString. ---- */
typedef size_t (*lz4f_mi355x_await_fn)(void* user, const void** data);
/* compress = compressWithOutBufferSize 0 (Conduit.hsc:336-337, :457-533); prefs NULL = lz4DefaultPreferences */
LZ4F_MI355X_API int lz4f_mi355x_conduit_compress(size_t outBufferSize, const LZ4F_preferences_t* prefs,
                                                 lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                 char* errbuf, size_t errcap);
/* compressYieldImmediately (Conduit.hsc:364-425) */
LZ4F_MI355X_API int lz4f_mi355x_conduit_compress_yield_immediately(const LZ4F_preferences_t* prefs,
                                                 lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                 char* errbuf, size_t errcap);
/* decompress (Conduit.hsc:598-701) */
LZ4F_MI355X_API int lz4f_mi355x_conduit_decompress(lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                 char* errbuf, size_t errcap);
/* batched conduits (new): gather >= batchBytes of input per GPU call */
LZ4F_MI355X_API int lz4f_mi355x_conduit_compress_batched(size_t batchBytes, const LZ4F_preferences_t* prefs,
                                                 lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                 char* errbuf, size_t errcap);
/* the same, and behind the frame its BLOCK LIST as a skippable frame (see lz4f_mi355x_appendBlockList): `mi355x-lz4c --index` */
LZ4F_MI355X_API int lz4f_mi355x_conduit_compress_batched_listed(size_t batchBytes, const LZ4F_preferences_t* prefs,
                                                 lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                 char* errbuf, size_t errcap);
LZ4F_MI355X_API int lz4f_mi355x_conduit_decompress_batched_bounded(size_t batchBytes, lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                                  char* errbuf, size_t errcap);
LZ4F_MI355X_API int lz4f_mi355x_conduit_decompress_batched(lz4f_mi355x_await_fn await, lz4f_mi355x_yield_fn yield, void* user,
                                                 char* errbuf, size_t errcap);

#ifdef __cplusplus
}
#endif
#endif /* LZ4F_MI355X_H */
