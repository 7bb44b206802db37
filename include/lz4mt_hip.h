/*
 * lz4mt_hip.h — MI355X extensions to the lz4mt C ABI (liblz4mt_amd.so).
 *
 * Three layers, all plain C types (pointers, sizes, an opaque stream):
 *
 * 1. Block operators with exactly the reference's plugin signatures
 *    (typedefs Lz4MtCompress / Lz4MtCompressBound / Lz4MtDecompress,
 *    reference src/lz4mt.h:41-58).  Assign them to ctx.compress /
 *    ctx.compressBound / ctx.decompress and the reference-shaped host
 *    scheduler (lz4mtCompress in PARALLEL/SEQUENTIAL mode) runs every block
 *    on the GPU.  Host pointers; each call stages through device memory.
 *    They replace LZ4_compress_limitedOutput / LZ4_compressBound /
 *    LZ4_decompress_safe as wired in reference src/main.cpp:749-751,767-785.
 *
 * 2. Device-resident frame engine: one call compresses or decompresses a
 *    whole lz4mt frame whose input and output already live in HBM
 *    (the performance path; used by lz4mtCompress/lz4mtDecompress in
 *    LZ4MT_MODE_DEVICE and by bench.py).
 *
 * 3. Utilities: synthetic input generator, XXH32, device info.
 *
 * Streams are hipStream_t passed as void* (NULL = default stream).
 * Every function fails loudly (returns LZ4MT_RESULT_ERROR / a negative
 * value) when no HIP device is present; nothing falls back to the CPU.
 */
#ifndef LZ4MT_AMD_LZ4MT_HIP_H
#define LZ4MT_AMD_LZ4MT_HIP_H

#include "lz4mt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. block operators (reference plugin signatures) ------------------ */
/* LZ4_compress_limitedOutput semantics (lz4 1.9.3, acceleration 1):
 * returns the compressed size, or 0 when it does not fit maxOutputSize.
 * compressionLevel >= 3: LZ4_compressHC2_limitedOutput, the codec the
 * reference wires for those levels (src/main.cpp:778-785): 3..9 LZ4-HC
 * 1.9.3's hash-chain parser, 10..12 its optimal parser
 * (LZ4HC_compress_optimal); levels above 12 are clamped to 12 as lz4hc
 * does. */
int lz4mtHipCompressBlock(const char* src, char* dst, int isize, int maxOutputSize, int compressionLevel);
/* LZ4_compressBound. */
int lz4mtHipCompressBound(int isize);
/* LZ4_decompress_safe semantics: decoded size, or a negative value. */
int lz4mtHipDecompressBlock(const char* src, char* dst, int isize, int maxOutputSize);

/* ---- 2. device-resident frame engine ----------------------------------- */
/* Upper bound of a frame for srcSize input bytes under `sd`. */
uint64_t lz4mtHipFrameBound(uint64_t srcSize, const Lz4MtStreamDescriptor* sd);
/* Scratch bytes lz4mtHipCompressFrame needs for srcSize (slots + tables). */
uint64_t lz4mtHipCompressWorkspaceSize(uint64_t srcSize, const Lz4MtStreamDescriptor* sd);
/* Compresses d_src[0..srcSize) into one frame at d_frame (device memory).
 * d_workspace may be NULL (the library then allocates and frees scratch).
 * *frameSize (host) receives the frame length; the call synchronises the
 * stream once at the end to read it.  blockIndependence = 0 writes a
 * block-dependent (-BD) frame: one wavefront encodes the blocks in order,
 * each against the 64 KiB before it (lz4's streaming compressor, as the
 * reference's compressBlockDependency calls it).  The plan, table and
 * round scratch of -BD frames live in the workspace, so size it with
 * lz4mtHipCompressWorkspaceSize for the same `sd`. */
Lz4MtResult lz4mtHipCompressFrame(const void* d_src, uint64_t srcSize, void* d_frame, uint64_t frameCap,
                                  uint64_t* frameSize, const Lz4MtStreamDescriptor* sd,
                                  void* d_workspace, uint64_t workspaceSize, void* stream);
/* Asynchronous variant: *d_frameSize is device memory, nothing is
 * synchronised (the stream carries the dependency). */
Lz4MtResult lz4mtHipCompressFrameAsync(const void* d_src, uint64_t srcSize, void* d_frame, uint64_t frameCap,
                                       uint64_t* d_frameSize, const Lz4MtStreamDescriptor* sd,
                                       void* d_workspace, uint64_t workspaceSize, void* stream);

/* The same with a compression level: 0..2 fast LZ4, 3..9 LZ4-HC hash
 * chain, 10..12 (and above, clamped to 12) LZ4-HC's optimal parser (the
 * workspace then holds 2 more bytes per input byte: use
 * lz4mtHipCompressWorkspaceSizeEx).  Block-dependent frames at any level
 * >= 3 are the reference's HC stream, which runs at lz4hc's level 9. */
uint64_t lz4mtHipCompressWorkspaceSizeEx(uint64_t srcSize, const Lz4MtStreamDescriptor* sd, int level);
Lz4MtResult lz4mtHipCompressFrameEx(const void* d_src, uint64_t srcSize, void* d_frame, uint64_t frameCap,
                                    uint64_t* frameSize, const Lz4MtStreamDescriptor* sd, int level,
                                    void* d_workspace, uint64_t workspaceSize, void* stream);
Lz4MtResult lz4mtHipCompressFrameAsyncEx(const void* d_src, uint64_t srcSize, void* d_frame, uint64_t frameCap,
                                         uint64_t* d_frameSize, const Lz4MtStreamDescriptor* sd, int level,
                                         void* d_workspace, uint64_t workspaceSize, void* stream);

/* Parses the frame header at d_frame (one small device->host copy) and
 * reports its descriptor, header length and an upper bound of the decoded
 * size (blocks x blockMax, from a device walk of the block size words). */
Lz4MtResult lz4mtHipFrameInfo(const void* d_frame, uint64_t frameSize, Lz4MtStreamDescriptor* sd,
                              uint64_t* decodedBound, uint64_t* nBlocks, void* stream);
/* Decompresses every frame in d_frame[0..frameSize) (concatenated frames
 * and skippable frames included) into d_out.  outCap must hold
 * (blocks x blockMax) bytes of the last frame (see lz4mtHipFrameInfo).
 * *outSize receives the decoded length; `sd` the last frame's descriptor.
 * Result codes follow lz4mtDecompress (reference src/lz4mt.cpp:938-1011). */
Lz4MtResult lz4mtHipDecompressFrame(const void* d_frame, uint64_t frameSize, void* d_out, uint64_t outCap,
                                    uint64_t* outSize, Lz4MtStreamDescriptor* sd, void* stream);

/* Upper bound of the decoded size of every frame in d_frame[0..frameSize)
 * (concatenated and skippable frames included): the out capacity
 * lz4mtHipDecompressFrame needs.  Walks each frame's size words. */
Lz4MtResult lz4mtHipStreamBound(const void* d_frame, uint64_t frameSize, uint64_t* decodedBound, void* stream);
/* Record table of the single frame at d_frame: recordStart[i] = frame
 * offset of block i's size word (i < *nBlocks), recordStart[*nBlocks] = the
 * EOS word; *hdrLen = header bytes incl. magic.  `cap` entries of host
 * memory (>= blocks + 1; recordStart NULL = count only).  The device walk of
 * lz4mtHipDecompressFrame; used to cut a frame into per-GPU sub-frames of
 * whole records (the multi-GPU decompress scatter). */
Lz4MtResult lz4mtHipFrameRecords(const void* d_frame, uint64_t frameSize, uint64_t* recordStart, uint64_t cap,
                                 uint64_t* nBlocks, int* hdrLen, Lz4MtStreamDescriptor* sd, void* stream);

/* ---- 3. utilities ------------------------------------------------------- */
/* SURVEY.md App. F generator, bit-identical to the CPU oracle. */
int lz4mtHipGenSynthetic(void* d_dst, uint64_t n, uint64_t seed, void* stream);
/* XXH32 (seed 0) of device memory; synchronises the stream.  One serial
 * chain (one wavefront): use it for small ranges. */
uint32_t lz4mtHipXxh32(const void* d_src, uint64_t len, void* stream);
/* XXH32 of each consecutive chunkBytes piece of d_src (the last one short)
 * into d_digests[ceil(len / chunkBytes)] (device memory), in parallel;
 * asynchronous.  Returns 0, or -1 without a device / on bad arguments. */
int lz4mtHipXxh32Chunks(const void* d_src, uint64_t len, uint32_t chunkBytes, uint32_t* d_digests, void* stream);
/* Number of HIP devices visible (0 = none: every compute entry point errors). */
int lz4mtHipDeviceCount(void);
/* Frees the calling thread's cached engine memory (the DEVICE mode's pinned
 * staging slots and device buffers, the decode scratch) and the idle
 * scratch of the block operators.  LZ4MT_MODE_DEVICE callers keep their
 * slots between calls (no re-pinning); relinked default-PARALLEL callers
 * have them freed at the end of every call. */
void lz4mtHipReleaseCaches(void);

/* Per-stage device timings (ms, hipEvents) of the last frame call on this
 * thread: [0] encode/decode kernel, [1] checksum kernel(s), [2] scan +
 * assemble / walk + verify, [3] whole call.  Enabled by
 * lz4mtHipSetTiming(1) (adds event records, no synchronisation). */
void lz4mtHipSetTiming(int enable);
int lz4mtHipGetTimings(float* ms4);

/* ---- 4. block-sharded multi-GPU compress, gather streamed beside the encode
 * (lz4mt_amd/dist.py drives it over RCCL).  A shard is a
 * contiguous block range of one -Sx stream (FLG.2 and FLG.3 off: they do not
 * shard).  The sending rank launches its encode once, then packs rounds of
 * whatever the encoder has published so far (each round one contiguous
 * buffer: header, a descriptor per block, payload) and sends them while the
 * encode runs; the root unpacks them into a mirror of that shard's slots and,
 * once every shard is complete, assembles each shard's records into the one
 * frame.  Replaces nothing in the reference (it has no multi-device path);
 * the frame is the one lz4mtCompress writes for the whole stream
 * (src/lz4mt.cpp:898-935). ------------------------------------------------ */
/* Bytes of a shard workspace, and of the root's mirror of a shard (same
 * layout); 0 for a descriptor that cannot shard. */
uint64_t lz4mtHipShardWorkspaceSize(uint64_t n, const Lz4MtStreamDescriptor* sd);
/* Largest pack one round can produce with at most perBlockCap bytes per block. */
uint64_t lz4mtHipShardPackBound(uint64_t n, const Lz4MtStreamDescriptor* sd, uint32_t perBlockCap);
/* The frame header lz4mtCompress writes for `sd` (magic .. header checksum)
 * into out[19]; returns its length, -1 on a bad descriptor. */
int lz4mtHipFrameHeader(const Lz4MtStreamDescriptor* sd, uint8_t* out);
/* Zeroes the workspace's round state (published, packed and hashed counts)
 * on `stream`.  Required before every encode into the workspace, and it must
 * be stream-ordered before the encode AND before the call's first pack (the
 * two usually run on different streams: reset on a stream both wait on). */
Lz4MtResult lz4mtHipShardReset(uint64_t n, const Lz4MtStreamDescriptor* sd, void* d_ws, uint64_t wsSize, void* stream);
/* Launches the shard's encode (+ block checksums) on `stream`; 1 and 4 MiB
 * blocks publish their progress as they go.  Asynchronous.  The workspace
 * must have been reset (lz4mtHipShardReset) after its previous use. */
Lz4MtResult lz4mtHipShardEncode(const void* d_src, uint64_t n, const Lz4MtStreamDescriptor* sd, void* d_ws,
                                uint64_t wsSize, void* stream);
/* Forgets the call-order state kept for the workspace at d_ws (its next use
 * needs lz4mtHipShardReset first).  Call it when the workspace is freed, so
 * that a new allocation at the same address starts unknown. */
void lz4mtHipShardRelease(const void* d_ws);
/* One round into d_pack (capacity >= lz4mtHipShardPackBound): final = 0 while
 * the encode may still run (stream-ordered anywhere), final = 1 once it is
 * done (stream-ordered after it; repeat until the header's flags bit 0 is
 * set).  Header (64 B, little-endian): u64 magic, u64 payload bytes, u64
 * bytes still to send, u64 bytes of this pack, u32 blocks, u32 flags
 * (1 = shard complete), u64 the shard's record bytes (when complete). */
Lz4MtResult lz4mtHipShardPack(const void* d_src, uint64_t n, const Lz4MtStreamDescriptor* sd, void* d_ws,
                              uint64_t wsSize, void* d_pack, uint64_t packCap, uint32_t perBlockCap, int final,
                              void* stream);
/* Root: one received pack of an n-byte shard into its mirror (a buffer of
 * lz4mtHipShardWorkspaceSize bytes). */
Lz4MtResult lz4mtHipShardUnpack(const void* d_pack, uint64_t n, const Lz4MtStreamDescriptor* sd, void* d_mirror,
                                uint64_t mirrorSize, void* stream);
/* The shard's records (size word, payload, [checksum]) into d_body, as they
 * stand in the frame of the whole stream.  d_ws: a complete mirror, or the
 * shard workspace itself after its encode; d_src: the shard's source for the
 * latter (incompressible blocks), NULL for a mirror.  Body bytes = the
 * complete pack's record bytes. */
Lz4MtResult lz4mtHipShardAssemble(const void* d_src, uint64_t n, const Lz4MtStreamDescriptor* sd, void* d_ws,
                                  uint64_t wsSize, void* d_body, uint64_t bodyCap, void* stream);
/* The root's receive buffers for the copy-engine push of packs: allocate
 * (hipMalloc) and export an IPC handle (64 bytes); open / close another
 * process's buffer (mapped for the calling thread's device); free; and an
 * asynchronous device-to-device copy (a mapped peer buffer included).
 * 0 on success, -1 otherwise. */
int lz4mtHipIpcAlloc(uint64_t bytes, void** d_ptr, void* handle64);
/* The same, choosing the memory kind (*kind receives it): 2 uncached device
 * memory (hipDeviceMallocUncached: no L2 line of it is ever held, so a peer
 * copy engine's writes are what every later read sees), 1 fine-grained,
 * 0 plain hipMalloc -- the best kind <= want that allocates and exports an
 * IPC handle.  lz4mtHipShardUnpack starts with a system-scope acquire in
 * every case. */
int lz4mtHipIpcAllocKind(uint64_t bytes, void** d_ptr, void* handle64, int want, int* kind);
/* PCI bus id ("dddd:bb:dd.f", len >= 13) of device `dev`; the ordinal of the
 * visible device with that bus id (-1: not visible); hipDeviceCanAccessPeer
 * (1 yes, 0 no, -1 error).  The IPC setup identifies the root's GPU by bus id
 * so that processes that number devices differently agree. */
int lz4mtHipDevicePciBusId(int dev, char* buf, int len);
int lz4mtHipDeviceByPciBusId(const char* busId);
int lz4mtHipCanAccessPeer(int dev, int peer);
int lz4mtHipIpcOpen(const void* handle64, void** d_ptr);
int lz4mtHipIpcClose(void* d_ptr);
int lz4mtHipFree(void* d_ptr);
int lz4mtHipCopyAsync(void* d_dst, const void* d_src, uint64_t n, void* stream);
/* Record bytes of a complete shard workspace (or mirror): synchronises the
 * stream; UINT64_MAX on bad arguments or a device error. */
uint64_t lz4mtHipShardBodyBytes(uint64_t n, const Lz4MtStreamDescriptor* sd, void* d_ws, uint64_t wsSize, void* stream);

/* ---- 5. batched block operators (device memory) ------------------------- */
/* Many independent raw LZ4 blocks ("chunks") that already live in HBM, one
 * launch per call, one wavefront per chunk.  Chunk i is d_srcPtrs[i]
 * [0, d_srcSizes[i]) and goes to d_dstPtrs[i] [0, d_dstCaps[i]); its outcome
 * is d_outSizes[i].
 * All pointers are device pointers; `stream` is a hipStream_t as void*.
 * Asynchronous: no host synchronisation, no allocation, no host read of the
 * arrays -- so both calls can be captured into a HIP graph (a compress call
 * captured before any uncaptured call has checked the device's encoder
 * order takes the read-back probe, as the frame engine does: same bytes).
 *
 * Compress (the fast codec, level 0): bytes and d_outSizes[i] are those of
 * lz4mtHipCompressBlock(src, dst, d_srcSizes[i], d_dstCaps[i], 0), i.e.
 * LZ4_compress_limitedOutput of lz4 1.9.3 -- 0 when the block does not fit.
 * d_dstCaps == NULL: every capacity is lz4mtHipCompressBound(d_srcSizes[i]).
 * A size of 0 is valid (the one-token block).  maxChunkBytes is the caller's
 * promise d_srcSizes[i] <= maxChunkBytes <= LZ4MT_HIP_BATCH_MAX_CHUNK; it
 * selects the kernel (below 65 547: the byU16-only one).
 * Decompress: bytes and d_outSizes[i] are those of
 * lz4mtHipDecompressBlock(src, dst, d_srcSizes[i], d_dstCaps[i]), i.e.
 * LZ4_decompress_safe -- negative for a malformed block.  d_dstCaps[i] may
 * be anything from 0 up (a size or capacity above INT32_MAX gives -1, that
 * call's answer to a negative int); bytes of dst past the returned size are
 * unspecified.
 *
 * Memory: sources at any alignment, a chunk may end on the last byte of its
 * allocation (no source dword outside the chunk is read); destinations
 * 16-byte aligned; nothing is written at or beyond dst + cap.
 * d_outSizes[i] = LZ4MT_HIP_BATCH_BAD_CHUNK, and nothing written, for a
 * chunk with a null or misaligned destination, a null source of non-zero
 * size, or (compress) a size above maxChunkBytes.
 *
 * LZ4MT_RESULT_BAD_ARG: a null array with nChunks > 0 (d_dstCaps may be
 * null for compress only), maxChunkBytes above the maximum; then
 * LZ4MT_RESULT_ERROR without a HIP device or on a launch error; else
 * LZ4MT_RESULT_OK (nChunks == 0 launches nothing).
 *
 * Compress with a level (lz4mtHipCompressBatchEx).  level < 3: exactly
 * lz4mtHipCompressBatch; the workspace is ignored and may be NULL.
 * level >= 3: LZ4-HC.  Bytes and d_outSizes[i] are those of
 * lz4mtHipCompressBlock(src, dst, d_srcSizes[i], d_dstCaps[i], level), i.e.
 * LZ4_compressHC2_limitedOutput of lz4 1.9.3 (levels 3..9 the hashChain
 * parser, 10..12 the optimal parser, above 12 = 12) -- 0 when the block does
 * not fit; d_dstCaps == NULL as above.  The blocks are ordinary LZ4 blocks:
 * lz4mtHipDecompressBatch decodes them.  The memory contract and the refused
 * chunks (LZ4MT_HIP_BATCH_BAD_CHUNK) are the same as for the fast codec.
 * One wavefront parses one chunk from end to end, whatever its size: the
 * frame engine's split parse of 1 and 4 MiB blocks is not used here.
 * Workspace: device scratch in slots sized by maxChunkBytes (2 bytes per
 * source byte for the hash chain; from level 10 up a 57 KiB price table as
 * well); slot k serves the k-th chunk of a round.
 * lz4mtHipCompressBatchWorkspaceSize(maxChunkBytes, nChunks, level) is
 * min(nChunks, LZ4MT_HIP_BATCH_HC_SLOTS) slots -- with nChunks = 1, one slot,
 * which is never 0 at level >= 3 -- and 0 at level < 3.  The call accepts any
 * 256-byte-aligned workspace of at least one slot, uses
 * min(workspaceSize / slot, LZ4MT_HIP_BATCH_HC_SLOTS) slots and runs
 * ceil(nChunks / slots) rounds of two launches on `stream`: a smaller
 * workspace costs time, never bytes.  The workspace must not be used by
 * anything else until the call has run; its contents need not be kept.
 * Still asynchronous and graph-capturable: no allocation, no
 * synchronisation, no host read of the arrays, no environment variable.
 * LZ4MT_RESULT_BAD_ARG as above, then (level >= 3 and nChunks > 0) for a
 * workspace that is NULL, not 256-byte aligned or smaller than one slot. */
#define LZ4MT_HIP_BATCH_MAX_CHUNK (4u << 20)
#define LZ4MT_HIP_BATCH_BAD_CHUNK INT32_MIN
#define LZ4MT_HIP_BATCH_HC_SLOTS 16384u
Lz4MtResult lz4mtHipCompressBatch(const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes,
                                  uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps,
                                  int32_t* d_outSizes, void* stream);
uint64_t lz4mtHipCompressBatchWorkspaceSize(uint32_t maxChunkBytes, uint32_t nChunks, int level);
Lz4MtResult lz4mtHipCompressBatchEx(const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes,
                                    uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps,
                                    int32_t* d_outSizes, int level, void* d_workspace, uint64_t workspaceSize,
                                    void* stream);
Lz4MtResult lz4mtHipDecompressBatch(const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t nChunks,
                                    void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes,
                                    void* stream);

/* ---- 5b. the batched operators with a shared dictionary -------------------
 * Small chunks compress badly on their own: each starts with an empty table
 * and no history.  These calls give every chunk of a batch the same
 * dictionary, as lz4's LZ4_loadDict + LZ4_compress_fast_continue and
 * LZ4_decompress_safe_usingDict do.  Everything is device memory; all three
 * calls are asynchronous, allocate nothing, synchronise nothing and read no
 * device memory on the host: graph-capturable exactly as the calls above
 * (including the compress call's read-back probe when captured first).
 *
 * State: lz4mtHipDictStateSize() bytes (a constant, a multiple of 256: the
 * 16 KiB table plus a small header), opaque, 256-byte aligned.
 * lz4mtHipDictPrepare builds it with one kernel: the table LZ4_loadDict
 * leaves, and the effective dictionary size.  The dictionary may stand at
 * any alignment and end on the last byte of its allocation.  The effective
 * dictionary is the last min(dictSize, LZ4MT_HIP_DICT_WINDOW) bytes, and
 * none at all when dictSize < 8 (lz4's HASH_UNIT).
 *
 * Compress: bytes and d_outSizes[i] are those of, on lz4 1.9.3 and with the
 * dictionary and the chunk in separate buffers (usingExtDict),
 *     LZ4_loadDict(stream, dict, dictSize);
 *     LZ4_compress_fast_continue(stream, src_i, dst_i, size_i, cap_i, 1);
 * -- 0 when the block does not fit.  Without an effective dictionary that is
 * still a fresh lz4 *stream* (byU32 table at any size), so chunks below
 * 65 547 bytes do not get lz4mtHipCompressBatch's byU16 bytes.
 * d_dstCaps == NULL, maxChunkBytes, the memory contract and the refused
 * chunks are those of lz4mtHipCompressBatch.  d_dict / dictSize must be what
 * d_state was prepared for: when the effective size differs from the one
 * the state records, every chunk gets LZ4MT_HIP_BATCH_BAD_CHUNK and nothing
 * is written (decided on the device; a guard against a stale state, not a
 * checksum of the dictionary).
 *
 * Decompress: bytes and d_outSizes[i] are those of
 * LZ4_decompress_safe_usingDict(src, dst, size, cap, dict, dictSize) with the
 * dictionary not adjacent to dst (every negative return included); with
 * dictSize == 0 those of lz4mtHipDecompressBatch.  It needs no state, and
 * the whole dictionary counts (offsets reach its last 65 535 bytes).
 *
 * LZ4MT_RESULT_BAD_ARG, in this order: a null array with nChunks > 0
 * (d_dstCaps may be null for compress only); maxChunkBytes above the
 * maximum; a null d_dict with dictSize > 0; (prepare, compress) a state
 * that is null, not 256-byte aligned or smaller than the state size.  Then
 * LZ4MT_RESULT_ERROR without a HIP device or on a launch error; else
 * LZ4MT_RESULT_OK (nChunks == 0 launches nothing). */
#define LZ4MT_HIP_DICT_WINDOW (64u << 10)
uint64_t lz4mtHipDictStateSize(void);
Lz4MtResult lz4mtHipDictPrepare(const void* d_dict, uint32_t dictSize, void* d_state, uint64_t stateSize,
                                void* stream);
Lz4MtResult lz4mtHipCompressBatchDict(const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes,
                                      uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps,
                                      int32_t* d_outSizes, const void* d_dict, uint32_t dictSize,
                                      const void* d_state, void* stream);
Lz4MtResult lz4mtHipDecompressBatchDict(const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t nChunks,
                                        void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes,
                                        const void* d_dict, uint32_t dictSize, void* stream);

/* ---- 5c. LZ4-HC (levels 3..12) with a shared dictionary --------------------
 * The dictionary of section 5b under the LZ4-HC parsers of
 * lz4mtHipCompressBatchEx: what small chunks gain most from.  The blocks are
 * ordinary LZ4 blocks; lz4mtHipDecompressBatchDict decodes them.
 *
 * Compress: bytes and d_outSizes[i] are those of, on lz4 1.9.3, with a fresh
 * LZ4_createStreamHC() stream per chunk and the dictionary, the source and
 * the destination in three separate, non-adjacent buffers (lz4hc's
 * external-dictionary mode),
 *     LZ4_resetStreamHC_fast(s, level);
 *     LZ4_loadDictHC(s, dict, dictSize);
 *     LZ4_compress_HC_continue(s, src_i, dst_i, size_i, cap_i);
 * -- 0 when the block does not fit (cap_i >= lz4mtHipCompressBound(size_i) is
 * lz4hc's notLimited path; d_dstCaps == NULL means that bound).  Levels are
 * 3..12, above 12 counts as 12.  The effective dictionary is the last
 * min(dictSize, LZ4MT_HIP_DICT_WINDOW) bytes.  These are not the bytes of a
 * dictionary and chunk laid out in one buffer (lz4hc's prefix mode).
 * A dictionary shorter than 4 bytes inserts nothing into lz4hc's tables and
 * gives the bytes of lz4mtHipCompressBatchEx at the same level (pinned
 * against liblz4 for the fixture's inputs, tests/golden/make_golden_dict_hc.py).
 * One point where liblz4 itself is not defined by its inputs: the optimal
 * parser (levels 10..12) can reach one of the dictionary's last three
 * positions as a match candidate, and lz4hc 1.9.3 then compares four bytes of
 * which up to three lie past the dictionary's end.  Here such a candidate
 * never matches, and no byte outside the dictionary is read; that is liblz4's
 * answer whenever the bytes behind its dictionary buffer do not happen to
 * continue the chunk.
 *
 * State: lz4mtHipDictStateSizeHC() bytes (a constant, a multiple of 256:
 * 32 768 hash heads, 65 536 chain links, a header and padding), opaque,
 * 256-byte aligned.  lz4mtHipDictPrepareHC builds it with one kernel,
 * asynchronously: what LZ4_loadDictHC leaves behind (the hash heads, the chain
 * links of the effective dictionary's inserted positions 0 .. size - 4, the
 * effective size).  It does not depend on the level: one state serves levels
 * 3..12.  It is not the state of section 5b, and neither call takes the
 * other's: lz4mtHipCompressBatchDictHC given a state built by
 * lz4mtHipDictPrepare, or lz4mtHipCompressBatchDict given one built by
 * lz4mtHipDictPrepareHC, refuses every chunk (LZ4MT_HIP_BATCH_BAD_CHUNK,
 * nothing written; decided on the device).  The same happens when the
 * effective size of dictSize differs from the one the state records (the
 * stale-state guard of section 5b).
 * The dictionary may stand at any alignment and end on the last byte of its
 * allocation; no byte outside its effective part, and no byte outside a
 * chunk, is read.
 *
 * Workspace: lz4mtHipCompressBatchDictWorkspaceSize(maxChunkBytes, nChunks,
 * level) -- slots, rounds and rules as lz4mtHipCompressBatchEx: any 256-byte
 * aligned workspace of at least one slot (the size for nChunks = 1) is
 * accepted, min(workspaceSize / slot, LZ4MT_HIP_BATCH_HC_SLOTS) slots are
 * used in ceil(nChunks / slots) rounds; a smaller workspace costs time, never
 * bytes.  The memory contract and the refused chunks are those of
 * lz4mtHipCompressBatch.  Asynchronous and graph-capturable: no allocation,
 * no synchronisation, no host read of device memory, no environment variable.
 *
 * LZ4MT_RESULT_BAD_ARG, in this order: a null array with nChunks > 0
 * (d_dstCaps may be null); maxChunkBytes above the maximum; level < 3 (the
 * fast codec has its own call and its own state); a null d_dict with
 * dictSize > 0; a state that is null, not 256-byte aligned or (prepare)
 * smaller than the state size; with nChunks > 0 a workspace that is null, not
 * 256-byte aligned or smaller than one slot.  Then LZ4MT_RESULT_ERROR without
 * a HIP device or on a launch error; else LZ4MT_RESULT_OK (nChunks == 0
 * launches nothing). */
uint64_t lz4mtHipDictStateSizeHC(void);
Lz4MtResult lz4mtHipDictPrepareHC(const void* d_dict, uint32_t dictSize, void* d_state, uint64_t stateSize,
                                  void* stream);
uint64_t lz4mtHipCompressBatchDictWorkspaceSize(uint32_t maxChunkBytes, uint32_t nChunks, int level);
Lz4MtResult lz4mtHipCompressBatchDictHC(const void* const* d_srcPtrs, const uint32_t* d_srcSizes,
                                        uint32_t maxChunkBytes, uint32_t nChunks, void* const* d_dstPtrs,
                                        const uint32_t* d_dstCaps, int32_t* d_outSizes, const void* d_dict,
                                        uint32_t dictSize, const void* d_stateHC, int level, void* d_workspace,
                                        uint64_t workspaceSize, void* stream);

/* ---- 5d. a set of dictionaries, one index per chunk -------------------------
 * The operators of section 5b for a batch whose chunks belong to many
 * dictionaries (one per table, column, tenant, message type): one call, one
 * launch, whatever the number of dictionaries.  Dictionary k is
 * d_dictPtrs[k] [0, d_dictSizes[k]), at any alignment; it may end on the
 * last byte of its allocation, and the same dictionary may be listed more
 * than once.  Chunk i uses dictionary d_chunkDict[i], or none when that is
 * LZ4MT_HIP_BATCH_NO_DICT.  d_dictPtrs, d_dictSizes and d_chunkDict are
 * device arrays like the others and the host reads none of them: all three
 * calls allocate nothing, synchronise nothing and are graph-capturable
 * exactly as section 5b's.  The effective size of a dictionary (0 below 8
 * bytes, else min(size, LZ4MT_HIP_DICT_WINDOW)) and its end (pointer + size,
 * in 64-bit arithmetic) are computed on the device.
 *
 * States: state k stands at d_states + k * lz4mtHipDictStateSize(); d_states
 * is 256-byte aligned and statesSize >= nDicts * lz4mtHipDictStateSize().
 * lz4mtHipDictSetPrepare builds them all with one launch.  State k is byte
 * for byte what lz4mtHipDictPrepare writes for dictionary k, and a state made
 * by either call is valid for the other.  A dictionary with a null pointer
 * and an effective size above 0 gets a state that no dictionary matches: the
 * compress call refuses its chunks.
 *
 * Compress: a chunk with k = d_chunkDict[i] < nDicts gets the bytes and
 * d_outSizes[i] of lz4mtHipCompressBatchDict called with dictionary k and
 * state k.  k == LZ4MT_HIP_BATCH_NO_DICT is the same without a dictionary
 * (section 5b with dictSize = 0: a fresh lz4 stream, byU32) and needs no
 * state.  LZ4MT_HIP_BATCH_BAD_CHUNK and nothing written, decided on the
 * device and with no effect on any other chunk of the call: the chunks
 * lz4mtHipCompressBatch refuses; an index >= nDicts other than
 * LZ4MT_HIP_BATCH_NO_DICT; a dictionary with a null pointer and a size above
 * 0; a state whose recorded size differs from the dictionary's effective
 * size (section 5b's stale-state guard, per chunk).  d_dstCaps == NULL,
 * maxChunkBytes and the memory contract are those of lz4mtHipCompressBatch.
 *
 * Decompress: chunk i is LZ4_decompress_safe_usingDict against the whole of
 * dictionary k, every negative return included; with
 * LZ4MT_HIP_BATCH_NO_DICT or a dictionary of size 0 it is
 * LZ4_decompress_safe (lz4mtHipDecompressBatch).  LZ4MT_HIP_BATCH_BAD_CHUNK
 * for an index that names no dictionary or a dictionary with a null pointer
 * and a size above 0, and for the chunks lz4mtHipDecompressBatch refuses.  It
 * needs no states, and decodes LZ4-HC blocks as section 5b's decoder does.
 *
 * LZ4-HC *compress* with a set of dictionaries is not part of this section:
 * its state is some 256 KiB per dictionary and its kernels are section 5c's.
 * It is the follow-up of section 5e (lz4mtHipCompressBatchDictSetHC), which
 * replaces one lz4mtHipCompressBatchDictHC call per dictionary; the blocks
 * either makes are decoded by the call below.
 *
 * LZ4MT_RESULT_BAD_ARG, in this order: a null chunk array with nChunks > 0
 * (d_chunkDict counts as one; d_dstCaps may be null for compress only);
 * maxChunkBytes above the maximum; a null d_dictPtrs or d_dictSizes with
 * nDicts > 0; (prepare, compress, with nDicts > 0) d_states null or not
 * 256-byte aligned, (prepare) or statesSize too small.  Then
 * LZ4MT_RESULT_ERROR without a HIP device or on a launch error; else
 * LZ4MT_RESULT_OK.  nDicts == 0 is valid (every chunk must then name
 * LZ4MT_HIP_BATCH_NO_DICT); nChunks == 0, or nDicts == 0 in prepare,
 * launches nothing. */
#define LZ4MT_HIP_BATCH_NO_DICT UINT32_MAX
Lz4MtResult lz4mtHipDictSetPrepare(const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts,
                                   void* d_states, uint64_t statesSize, void* stream);
Lz4MtResult lz4mtHipCompressBatchDictSet(const void* const* d_srcPtrs, const uint32_t* d_srcSizes,
                                         uint32_t maxChunkBytes, uint32_t nChunks, void* const* d_dstPtrs,
                                         const uint32_t* d_dstCaps, int32_t* d_outSizes,
                                         const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts,
                                         const void* d_states, const uint32_t* d_chunkDict, void* stream);
Lz4MtResult lz4mtHipDecompressBatchDictSet(const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t nChunks,
                                           void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes,
                                           const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts,
                                           const uint32_t* d_chunkDict, void* stream);

/* ---- 5e. LZ4-HC (levels 3..12) with a set of dictionaries -------------------
 * Section 5c's compressor behind section 5d's set: one call for a batch whose
 * chunks belong to many dictionaries, two launches per round whatever their
 * number.  d_dictPtrs, d_dictSizes and d_chunkDict are as in section 5d:
 * device arrays the host never reads, dictionary k at any alignment and free
 * to end on the last byte of its allocation, the same dictionary listed as
 * often as wanted, LZ4MT_HIP_BATCH_NO_DICT for a chunk without one.  Both
 * calls are asynchronous, allocate nothing, synchronise nothing, read no
 * environment variable and are graph-capturable.  The effective size of a
 * dictionary is min(size, LZ4MT_HIP_DICT_WINDOW) -- lz4hc's rule: there is no
 * 8-byte minimum here, and a size below 4 inserts nothing -- and its end is
 * pointer + size in 64-bit arithmetic; both are computed on the device.
 *
 * States: state k stands at d_statesHC + k * lz4mtHipDictStateSizeHC();
 * d_statesHC is 256-byte aligned and statesSize >= nDicts *
 * lz4mtHipDictStateSizeHC() (a 64-bit product).  lz4mtHipDictSetPrepareHC
 * builds them with one workgroup per dictionary, in a bounded number of
 * launches whatever nDicts is.  State k is byte for byte what
 * lz4mtHipDictPrepareHC writes for dictionary k, and a state made by either
 * call serves the other.  A dictionary with a null pointer and a size above 0
 * gets a state that no dictionary matches; a null pointer with size 0 is a
 * valid empty dictionary.
 *
 * Compress: a chunk with k = d_chunkDict[i] < nDicts gets the bytes and
 * d_outSizes[i] of lz4mtHipCompressBatchDictHC called with dictionary k,
 * state k and `level`.  k == LZ4MT_HIP_BATCH_NO_DICT gets the bytes of
 * lz4mtHipCompressBatchEx at `level` and needs no state: nDicts == 0 with
 * d_statesHC == NULL is valid (every chunk must then name
 * LZ4MT_HIP_BATCH_NO_DICT).  LZ4MT_HIP_BATCH_BAD_CHUNK and nothing written,
 * decided on the device, per chunk and with no effect on any other chunk of
 * the call: the chunks lz4mtHipCompressBatch refuses; an index >= nDicts
 * other than LZ4MT_HIP_BATCH_NO_DICT; a dictionary with a null pointer and a
 * size above 0; a state that is not an HC state for that dictionary's
 * effective size (stale, unprepared, or a state of section 5b / 5d).  Levels,
 * d_dstCaps == NULL and the memory contract are those of section 5c: no byte
 * outside a dictionary's effective part, and no byte outside a chunk, is
 * read.  lz4mtHipDecompressBatchDictSet decodes the blocks.
 *
 * Workspace: lz4mtHipCompressBatchDictWorkspaceSize(maxChunkBytes, nChunks,
 * level), the slots and rounds of section 5c: any 256-byte-aligned workspace
 * of at least one slot is accepted, and a smaller one costs time, never
 * bytes.  A round takes its slice of d_chunkDict with the other chunk arrays.
 *
 * LZ4MT_RESULT_BAD_ARG, in this order: a null chunk array with nChunks > 0
 * (d_chunkDict counts as one; d_dstCaps may be null); maxChunkBytes above the
 * maximum; level < 3; a null d_dictPtrs or d_dictSizes with nDicts > 0; with
 * nDicts > 0, d_statesHC null or not 256-byte aligned, (prepare) or
 * statesSize too small; with nChunks > 0 a workspace that is null, not
 * 256-byte aligned or smaller than one slot.  Then LZ4MT_RESULT_ERROR without
 * a HIP device or on a launch error; else LZ4MT_RESULT_OK.  nChunks == 0, or
 * nDicts == 0 in prepare, launches nothing. */
Lz4MtResult lz4mtHipDictSetPrepareHC(const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts,
                                     void* d_statesHC, uint64_t statesSize, void* stream);
Lz4MtResult lz4mtHipCompressBatchDictSetHC(const void* const* d_srcPtrs, const uint32_t* d_srcSizes,
                                           uint32_t maxChunkBytes, uint32_t nChunks, void* const* d_dstPtrs,
                                           const uint32_t* d_dstCaps, int32_t* d_outSizes,
                                           const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts,
                                           const void* d_statesHC, const uint32_t* d_chunkDict, int level,
                                           void* d_workspace, uint64_t workspaceSize, void* stream);

/* ---- 6. diagnostics ----------------------------------------------------- */
/* Runs s_memtime-stamped twins of the encode / decode kernels (never the
 * product launch) and sums per-phase shader cycles over all blocks.
 * encode (16 slots): [hash, table+dedup, candidate check, round issue,
 * literal staging, round wait, table writes, count, emit, loop overhead,
 * windows, tag aliases, tag-candidate winners, -, -, -];
 * decode (16 slots): [batch parse, serial literal copy, serial match copy
 * / batch dependent copies, batch group + far copies, batches, total,
 * matches, far matches, batch sequences, serial-path sequences, -...]. */
int lz4mtHipDebugEncodeStats(const void* d_src, uint64_t n, uint32_t blockSize, uint64_t* stats16, void* stream);
/* The same counters per block, unsummed: perBlock16 holds ceil(n /
 * blockSize) x 16 words (block b at 16 b).  0, or -1. */
int lz4mtHipDebugEncodeBlockStats(const void* d_src, uint64_t n, uint32_t blockSize, uint64_t* perBlock16,
                                  void* stream);
/* The frame path's block encoder alone over blocks of any size 65 547 B ..
 * 4 MiB (frames use 64 KiB .. 4 MiB by 4x steps; the others are timing
 * points of a split parse, tools/occ_sweep.py).  d_slots: nb x blockSize +
 * 64 bytes, d_csize: nb int32.  Asynchronous; 0, or -1 on bad arguments. */
int lz4mtHipDebugEncode(const void* d_src, uint64_t n, uint32_t blockSize, void* d_slots, void* d_csize, void* stream);
/* 1 when the current device applies one wave's same-address LDS exchanges
 * in ascending lane order (what the block encoders' exchange probe relies
 * on; checked once per device before the first encode), 0 when it does not
 * (the encoders then run their read-back probe: same bytes, no ordering
 * assumed), -1 without a device or when the check could not run. */
int lz4mtHipCheckEncoderOrder(void);
/* The table probe the block encoders use on the current device: 1 the LDS
 * exchange, 0 the read-back probe (the order check failed, or
 * LZ4MT_AMD_ENC_PROBE=readback), -1 without a device / on a HIP error.  A
 * call whose stream is being captured into a graph before this device was
 * checked also takes the read-back probe (the check synchronises). */
int lz4mtHipEncoderProbe(void);
/* The parse work of a split parse: n bytes in streams of S bytes, stream b
 * parsed from ov bytes before its start (the overlap a join needs), S + ov
 * <= 4 MiB, into d_slots (nb x (S + ov) + 64 bytes), sizes into d_csize;
 * p17 = 1 selects the 3-byte table.  Timing only; 0, or -1 on bad args. */
int lz4mtHipDebugEncodeOverlap(const void* d_src, uint64_t n, uint32_t S, uint32_t ov, int p17, void* d_slots,
                               void* d_csize, void* stream);
int lz4mtHipDebugDecodeStats(const void* d_frame, uint64_t frameSize, uint64_t* stats16, void* stream);
/* FETCH_SIZE calibration (tools/fetch_cal.py): reads n bytes of d_buf exactly
 * once with `width`-byte loads per lane (1, 4, 8 or 16); d_out4: 4 bytes of
 * device scratch.  Asynchronous; 0, or -1 on a bad width. */
/* The per-block lz4 stream plan of a -BD frame (host only): for blocks of
 * sizes[0..nBlocks), plan4[4b..4b+3] = catch-up bound for candidates in the
 * block, in the history, the dictSmall limit (block coordinates: the block
 * at 65536) and where the history bytes stand (0 = before the block; else
 * the block's own bytes from shift - 65536: the reference's buffer,
 * refBuffer = 1).  0 on success, 1 if a history would be neither, -1 on a
 * bad id. */
int lz4mtDebugBdPlan(int blockMaxId, int refBuffer, const uint32_t* sizes, uint64_t nBlocks, uint32_t* plan4);
int lz4mtHipDebugFetchCal(const void* d_buf, uint64_t n, int width, void* d_out4, void* stream);

#ifdef __cplusplus
}
#endif
#endif
