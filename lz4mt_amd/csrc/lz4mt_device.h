// lz4mt_device.h — shared declarations between the HIP kernels
// (lz4mt_kernels.hip) and the host engine (lz4mt_engine.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace lz4mt {

// LZ4 1.9.3 constants.
constexpr int kMinMatch = 4;
constexpr int kLastLiterals = 5;
constexpr int kMfLimit = 12;
constexpr int kMinLength = 13;
constexpr uint32_t kDistMax = 65535;
constexpr int kLimit64K = 65547;

// Decoder status codes beyond LZ4_decompress_safe's own negative values.
constexpr int kDecodeOutputTooSmall = INT32_MIN;   // physical slot smaller than the decoded block

// Batched block operators (lz4mt_hip.h section 5): the largest chunk, and the
// per-chunk status of a chunk the kernels refuse (LZ4MT_HIP_BATCH_BAD_CHUNK).
constexpr uint32_t kBatchMaxChunk = 4u << 20;
constexpr int32_t kBatchBadChunk = INT32_MIN;
// The same with a shared dictionary (section 5b): the window LZ4_loadDict
// keeps, its HASH_UNIT (sizeof(reg_t): a shorter dictionary is none), and the
// prepared state (the 16 KiB byU32 table + a 256-byte header whose first word
// is the effective dictionary size).
constexpr uint32_t kDictWindow = 64u << 10;
constexpr uint32_t kDictHashUnit = 8;
constexpr uint32_t kDictStateBytes = 16384 + 256;
// the compressor's effective dictionary: the last min(dictSize, 64 KiB) bytes, none below HASH_UNIT
__host__ __device__ inline uint32_t dict_effective(uint32_t dictSize) {
    return dictSize < kDictHashUnit ? 0u : (dictSize < kDictWindow ? dictSize : kDictWindow);
}
// A set of dictionaries with an index per chunk (sections 5d, 5e): the index
// of a chunk that has none (LZ4MT_HIP_BATCH_NO_DICT), and the size a set's
// prepare records, where a state keeps its effective size, for a dictionary
// that has a size and no pointer.  No effective size equals it, so the
// encoders' guards refuse the chunks that name such a state.
constexpr uint32_t kBatchNoDict = 0xFFFFFFFFu;
constexpr uint32_t kDictStateBad = 0xFFFFFFFFu;
static_assert(kDictStateBad > kDictWindow, "no effective size");

// The launchers of the batched operators: n chunks (or dictionaries) in grids
// of at most `grid`, launch(o, g) for the g items from o on; the first launch
// error ends it.  kBatchGrid: the most workgroups these launchers put in a grid.
constexpr uint32_t kBatchGrid = 1u << 30;
template <class F>
inline hipError_t launch_slices(uint32_t n, uint32_t grid, F&& launch) {
    for (uint32_t o = 0, g; o < n; o += g) {
        g = n - o < grid ? n - o : grid;
        launch(o, g);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

#ifdef __HIP__
// One chunk's descriptor, read at the uniform index blockIdx.x (scalar
// loads); bad: LZ4MT_HIP_BATCH_BAD_CHUNK, nothing written.  The one
// definition of a refused chunk for the fast kernels (lz4mt_kernels.hip) and
// the LZ4-HC ones (lz4mt_hc.hip).
struct BatchChunk {
    const __attribute__((address_space(1))) uint8_t* s;
    __attribute__((address_space(1))) uint8_t* d;
    uint32_t n, cap;
    bool bad;
};
__device__ __forceinline__ BatchChunk batch_chunk(const uint8_t* const* __restrict__ srcPtrs,
                                                  const uint32_t* __restrict__ srcSizes, uint32_t maxChunk,
                                                  uint8_t* const* __restrict__ dstPtrs,
                                                  const uint32_t* __restrict__ dstCaps) {
    const uint32_t i = blockIdx.x;
    BatchChunk c;
    c.n = srcSizes[i];
    const uint8_t* sp = srcPtrs[i];
    uint8_t* dp = dstPtrs[i];
    c.s = (const __attribute__((address_space(1))) uint8_t*)sp;
    c.d = (__attribute__((address_space(1))) uint8_t*)dp;
    c.cap = dstCaps ? dstCaps[i] : c.n + c.n / 255 + 16;   // lz4mtHipCompressBound
    c.bad = c.n > maxChunk || !dp || (reinterpret_cast<uintptr_t>(dp) & 15) != 0 || (!sp && c.n != 0);
    return c;
}
#endif

// Per-block record of a parsed frame (device-resident, one per block).
struct BlockRec {
    uint64_t offset;     // payload offset inside the frame
    uint32_t bits;       // size word: stored size | 0x80000000 if raw
    uint32_t checksum;   // block XXH32 read from the frame (if FLG.4)
};

// Per-block lz4 stream state of a block-dependent (-BD) frame's encode
// (see k_encode_linked): catch-up lower bounds for candidates in the block /
// in the history and the dictSmall limit, in coordinates where the block
// starts at 65536 and its 64 KiB history is [0, 65536).
// shift: where the history bytes stand (BdSim): 0 = the 64 KiB before the
// block; else position p < 65536 reads the block's own byte p - 65536 + shift
// (the reference's 1 / 4 MiB buffer, LZ4MT_AMD_BD_REFERENCE=1).
struct LinkPlan {
    uint32_t lowIn, lowDict, candLow, shift;
};

// Device state of a block-dependent encode: per-block plans, the carried table.
struct LinkState {
    LinkPlan* plan;
    uint32_t* table;
    bool fresh;
    uint32_t* rounds;    // parallel rounds' scratch, link_round_bytes(nBlocks) (null: the serial kernel)
    // level >= 3: the HC stream's segments (hc_bd_pack's layout on the device)
    const uint8_t* hcSegs = nullptr;
    uint32_t nSeg = 0;
    bool hcPerBlock = false;   // every block starts its own segment (1 / 4 MiB blocks)
    bool xh = false;           // some plan has a shift: the encoder variant that reads such histories
};

// Frame-walk summary written by the walk kernel.
struct WalkInfo {
    uint64_t endPos;     // position just after the EOS word
    uint32_t nBlocks;
    int32_t  result;     // Lz4MtResult code (0 = OK)
};

// Scratch of the parallel frame walk (launch_frame_walk_count/_path): the
// frame is scanned in 64 KiB chunks for candidate record offsets.
constexpr int kWalkChunkLog = 16;
struct WalkScratch {
    uint32_t* count;     // nChunks: candidates per chunk
    uint64_t* base;      // nChunks + 1: exclusive scan of count, M at [nChunks]
    uint64_t* pos;       // M: node -> frame offset (ascending)
    uint32_t* Ja;        // M + 1: successor tables (node M = DEAD)
    uint32_t* Jb;
    uint32_t* P;         // maxBlocks + 1 (path)
};

// A side stream + two events (per thread, re-made when the device changes)
// for work that can run beside the main stream.
struct AuxStream {
    hipStream_t st = nullptr;
    hipEvent_t evIn = nullptr, evMid = nullptr, evOut = nullptr;
    int dev = -1;
    bool ensure();
    void release();
    ~AuxStream() { release(); }
};

// ---- kernel launchers (lz4mt_kernels.hip) ----
// once per device, before the first block-encoder launch: the LDS exchange
// order the encoder's table probe relies on (k_xchg_order)
hipError_t encoder_ready(hipStream_t st);
hipError_t launch_encode_overlap(const uint8_t* src, uint64_t srcSize, uint32_t S, uint32_t ov, bool p17,
                                 uint8_t* slots, int32_t* csize, hipStream_t st);
hipError_t launch_encode(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                         uint8_t* slots, uint64_t slotStride, uint32_t capOverride, int32_t* csize,
                         hipStream_t st);
// k_encode with per-block progress publishing (pub[b]: bytes of slot b final;
// slot stride = blockSize), for the block-sharded streamed gather
hipError_t launch_encode_pub(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                             uint8_t* slots, int32_t* csize, uint32_t* pub, hipStream_t st);
hipError_t launch_decode(const uint8_t* frame, const BlockRec* recs, uint32_t nBlocks, uint32_t blockMax,
                         uint8_t* out, uint64_t outCap, int32_t* dsize, hipStream_t st);
// the batched block operators (k_encode_batch / k_encode_batch16 by maxChunk,
// k_decode_batch): one wave per chunk, every array in device memory,
// dstCaps null for the encode = the bound of each size
hipError_t launch_encode_batch(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t maxChunk,
                               uint32_t nChunks, uint8_t* const* dstPtrs, const uint32_t* dstCaps, int32_t* outSizes,
                               hipStream_t st);
hipError_t launch_decode_batch(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t nChunks,
                               uint8_t* const* dstPtrs, const uint32_t* dstCaps, int32_t* outSizes, hipStream_t st);
// the same with a shared dictionary (k_dict_prepare,
// k_encode_batch_dict<XC, SharedDict>, k_decode_batch_dict).  Encode: dictEnd is one past the dictionary's last
// byte and D = dict_effective(dictSize) bytes before it are the dictionary;
// state: kDictStateBytes, 256-byte aligned, written by launch_dict_prepare
// for the same D.  Decode: the whole dictionary counts (dictSize bytes
// before dictEnd; only the last 65535 can be reached); dictSize > 0.
hipError_t launch_dict_prepare(const uint8_t* dictEnd, uint32_t D, uint32_t* state, hipStream_t st);
hipError_t launch_encode_batch_dict(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t maxChunk,
                                    uint32_t nChunks, uint8_t* const* dstPtrs, const uint32_t* dstCaps,
                                    int32_t* outSizes, const uint8_t* dictEnd, uint32_t D, const uint32_t* state,
                                    hipStream_t st);
hipError_t launch_decode_batch_dict(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t nChunks,
                                    uint8_t* const* dstPtrs, const uint32_t* dstCaps, int32_t* outSizes,
                                    const uint8_t* dictEnd, uint32_t dictSize, hipStream_t st);
// the same with a set of dictionaries and an index per chunk (section 5d;
// k_dict_set_prepare, k_encode_batch_dict<XC, DictSet>, k_decode_batch_dict_set).
// dictPtrs / dictSizes / chunkDict are device arrays: the kernels compute the
// dictionary's end and dict_effective themselves.  State k stands at states +
// k * kDictStateBytes (256-byte aligned) and is what launch_dict_prepare
// writes for dictionary k.  chunkDict[i] = kBatchNoDict: no dictionary.
hipError_t launch_dict_set_prepare(const uint8_t* const* dictPtrs, const uint32_t* dictSizes, uint32_t nDicts,
                                   uint32_t* states, hipStream_t st);
hipError_t launch_encode_batch_dict_set(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t maxChunk,
                                        uint32_t nChunks, uint8_t* const* dstPtrs, const uint32_t* dstCaps,
                                        int32_t* outSizes, const uint8_t* const* dictPtrs, const uint32_t* dictSizes,
                                        uint32_t nDicts, const uint32_t* states, const uint32_t* chunkDict,
                                        hipStream_t st);
hipError_t launch_decode_batch_dict_set(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t nChunks,
                                        uint8_t* const* dstPtrs, const uint32_t* dstCaps, int32_t* outSizes,
                                        const uint8_t* const* dictPtrs, const uint32_t* dictSizes, uint32_t nDicts,
                                        const uint32_t* chunkDict, hipStream_t st);
// the serial frame walk fused with the decode (k_decode_walk): records are
// decoded as the walk publishes them.  ctl: 8 zeroed device words.
hipError_t launch_decode_walk(const uint8_t* frame, uint64_t frameSize, uint64_t bodyPos, uint32_t blockMax,
                              int blockChecksum, uint32_t maxBlocks, BlockRec* recs, WalkInfo* info, uint32_t* ctl,
                              uint8_t* out, uint64_t outCap, int32_t* dsize, uint32_t waves, hipStream_t st);
// beside it: the block checksums as the walk publishes them, and the verify
// with the walk's block count read on the device
hipError_t launch_xxh32_walked(const uint8_t* frame, const BlockRec* recs, uint32_t* ctl, uint32_t* digest,
                               uint32_t waves, hipStream_t st);
hipError_t launch_block_verify_walked(const BlockRec* recs, const WalkInfo* info, const uint32_t* digest,
                                      const int32_t* dsize, int blockChecksum, int32_t* status, uint32_t maxBlocks,
                                      hipStream_t st);
// the streamed compress's persistent encoder (lz4mt_kernels.hip, k_encode_stream);
// ticks: a wait's limit without progress (s_memrealtime, 100 MHz); pend:
// 4 words per wave, a block parked on its output slot (zeroed before the
// first launch of a call; a relaunch finishes those blocks first)
hipError_t launch_encode_stream(const uint8_t* hin, uint8_t* hout, uint32_t* inCtl, uint32_t* outCtl, uint32_t* g,
                                uint32_t* next, uint32_t* pend, uint8_t* dIn, uint8_t* dSlot, uint32_t bm, uint32_t Rin,
                                uint32_t Rout, uint32_t waves, int bck, uint64_t ticks, hipStream_t st);
// the streamed decompress's persistent decoder (lz4mt_kernels.hip, k_decode_stream)
hipError_t launch_decode_stream(const uint8_t* hin, uint8_t* hout, uint32_t* inCtl, uint32_t* outCtl, uint32_t* g,
                                uint32_t* next, uint32_t* pend, uint8_t* dIn, uint8_t* dSlot, uint32_t bm, uint32_t Rin,
                                uint32_t Rout, uint32_t waves, int bck, uint64_t ticks, hipStream_t st);
hipError_t launch_xxh32_stored(const uint8_t* src, const uint8_t* slots, uint64_t srcSize, uint32_t blockSize,
                               uint32_t nBlocks, const int32_t* csize, uint32_t* digest, hipStream_t st);
// block checksums while k_encode_pub runs (on another stream; pub / xdone
// zeroed before both), and the fix-up of blocks it did not finish
hipError_t launch_xxh32_follow(const uint8_t* src, const uint8_t* slots, uint64_t srcSize, uint32_t blockSize,
                               uint32_t nBlocks, uint32_t* pub, uint32_t* digest, uint32_t* xdone, hipStream_t st);
hipError_t launch_xxh32_fixup(const uint8_t* src, const uint8_t* slots, uint64_t srcSize, uint32_t blockSize,
                              uint32_t nBlocks, const int32_t* csize, uint32_t* digest, const uint32_t* xdone,
                              hipStream_t st);
hipError_t launch_xxh32_frame_blocks(const uint8_t* frame, const BlockRec* recs, uint32_t nBlocks, uint32_t* digest,
                                     hipStream_t st);
hipError_t launch_xxh32_stream(const uint8_t* p, uint64_t len, uint32_t* digest, hipStream_t st);
hipError_t launch_xxh32_chunks(const uint8_t* p, uint64_t len, uint32_t chunk, uint32_t* digest, hipStream_t st);
hipError_t launch_frame_scan(const int32_t* csize, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                             int blockChecksum, uint64_t* recOff, hipStream_t st);
hipError_t launch_frame_assemble(const uint8_t* src, const uint8_t* slots, uint64_t srcSize, uint32_t blockSize,
                                 uint32_t nBlocks, const int32_t* csize, const uint32_t* bsum,
                                 const uint64_t* recOff, int blockChecksum, uint8_t* frame, uint32_t hdrLen,
                                 hipStream_t st);
// blockChecksum for launch_frame_assemble: 0 none, 1 write the words, 2 leave
// them to launch_frame_sums
hipError_t launch_frame_sums(const int32_t* csize, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                             const uint32_t* bsum, const uint64_t* recOff, uint8_t* frame, uint32_t hdrLen,
                             hipStream_t st);
hipError_t launch_frame_finalize(uint8_t* frame, const uint8_t* hdr, uint32_t hdrLen, const uint64_t* recOff,
                                 uint32_t nBlocks, const uint32_t* streamSum, uint64_t* frameSize,
                                 hipStream_t st);
hipError_t launch_frame_walk(const uint8_t* frame, uint64_t frameSize, uint64_t bodyPos, uint32_t blockMax,
                             int blockChecksum, uint32_t maxBlocks, BlockRec* recs, WalkInfo* info,
                             hipStream_t st);
uint64_t frame_walk_par_chunks(uint64_t frameSize);
hipError_t launch_frame_walk_count(const uint8_t* frame, uint64_t frameSize, uint64_t bodyPos, uint32_t blockMax,
                                   int blockChecksum, const WalkScratch& ws, hipStream_t st);
hipError_t launch_frame_walk_path(const uint8_t* frame, uint64_t frameSize, uint64_t bodyPos, uint32_t blockMax,
                                  int blockChecksum, uint32_t maxBlocks, uint32_t M, const WalkScratch& ws,
                                  BlockRec* recs, WalkInfo* info, hipStream_t st);
hipError_t launch_block_verify(const BlockRec* recs, uint32_t nBlocks, const uint32_t* digest, const int32_t* dsize,
                               uint32_t blockMax, int blockChecksum, int32_t* status, hipStream_t st);
hipError_t launch_encode_stats(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                               uint8_t* slots, int32_t* csize, uint64_t* stats, hipStream_t st);
hipError_t launch_decode_stats(const uint8_t* frame, const BlockRec* recs, uint32_t nBlocks, uint32_t blockMax,
                               uint8_t* out, uint64_t outCap, int32_t* dsize, uint64_t* stats, hipStream_t st);
hipError_t launch_gen_synthetic(uint8_t* dst, uint64_t n, uint64_t seed, hipStream_t st);
// LZ4-HC (lz4mt_hc.hip): level 1..9 (lz4 1.9.3 hash chain); `delta` is
// scratch of 2 bytes per input byte.  hipErrorInvalidValue for levels > 9.
// capOverride: 0xFFFFFFFF = n (lz4mt), 0xFFFFFFFE = n - 1 (-BD), else the cap.
// splitWs (hc_split_bytes, or null): blocks of at least 2 x hc_split_sub()
// bytes are parsed by several waves and spliced (slotStride >= blockSize).
hipError_t launch_encode_hc(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                            uint8_t* slots, uint64_t slotStride, uint32_t capOverride, int level, uint16_t* delta,
                            int32_t* csize, hipStream_t st, uint8_t* splitWs = nullptr);
uint32_t hc_split_sub();
uint64_t hc_split_bytes(uint64_t nBlocks, uint32_t blockSize);
uint64_t hc_ws_bytes(uint64_t nBlocks, uint32_t blockSize, int level);   // splitWs size for a level
uint32_t hc_attempts(int level);   // lz4hc nbSearches of a level (> 12 = 12)
// The batched LZ4-HC (lz4mt_hip.h section 5, level >= 3): k_hc_prev_batch,
// then k_encode_hc_batch (levels 3..9) or k_encode_hc_opt_batch (10 and up),
// one wave per chunk, each a template over the chunk's dictionary source
// (here HcNoDict).  Scratch comes in slots of hc_batch_slot_bytes(maxChunk,
// level): the chunk's chain deltas and, from level 10 up, its price table;
// slot k serves the k-th chunk of a round.  ws holds `slots` >= 1 of them
// (256-byte aligned); the batch runs in ceil(nChunks / slots) rounds over
// slices of the arrays, a launch pair each, so a slot's next user starts
// after its previous one has ended.  kHcBatchSlots: the most slots a call
// uses (and lz4mtHipCompressBatchWorkspaceSize asks for): 16 waves for each
// of the 1024 SIMDs of an MI355X.
constexpr uint32_t kHcBatchSlots = 16384;
uint64_t hc_batch_slot_bytes(uint32_t maxChunk, int level);
hipError_t launch_encode_hc_batch(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t maxChunk,
                                  uint32_t nChunks, uint8_t* const* dstPtrs, const uint32_t* dstCaps,
                                  int32_t* outSizes, int level, uint8_t* ws, uint32_t slots, hipStream_t st);
// The same with a shared dictionary (section 5c; k_hc_dict_prepare, the
// batch kernels over HcSharedDict).
// LZ4_loadDictHC keeps the last 64 KiB whatever their number (below 4 bytes
// nothing is inserted, but the bytes still stand before the chunk).  The
// prepared state serves every level; its layout is lz4mt_hc.hip's.
constexpr uint32_t kHcDictMagic = 0x4C7E4843u;
constexpr uint32_t kHcDictHeadsAt = 16384 + 256;                       // behind the fast state's extent
constexpr uint32_t kHcDictLinksAt = kHcDictHeadsAt + (4u << 15);
constexpr uint32_t kHcDictStateBytes = kHcDictLinksAt + 2 * (kDictWindow + 128);
__host__ __device__ inline uint32_t hc_dict_effective(uint32_t dictSize) {
    return dictSize < kDictWindow ? dictSize : kDictWindow;
}
hipError_t launch_hc_dict_prepare(const uint8_t* dictEnd, uint32_t E, uint8_t* state, hipStream_t st);
hipError_t launch_encode_hc_batch_dict(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t maxChunk,
                                       uint32_t nChunks, uint8_t* const* dstPtrs, const uint32_t* dstCaps,
                                       int32_t* outSizes, const uint8_t* dictEnd, uint32_t E, const uint8_t* state,
                                       int level, uint8_t* ws, uint32_t slots, hipStream_t st);
// The same with a set of dictionaries and an index per chunk (section 5e;
// k_hc_dict_set_prepare, the batch kernels over HcDictSet).  dictPtrs / dictSizes / chunkDict are
// device arrays: the kernels compute the dictionary's end and its effective
// size themselves.  State k stands at states + k * kHcDictStateBytes (256-byte
// aligned) and is what launch_hc_dict_prepare writes for dictionary k.
// chunkDict[i] = kBatchNoDict: no dictionary (states may then be null).
hipError_t launch_hc_dict_set_prepare(const uint8_t* const* dictPtrs, const uint32_t* dictSizes, uint32_t nDicts,
                                      uint8_t* states, hipStream_t st);
hipError_t launch_encode_hc_batch_dict_set(const uint8_t* const* srcPtrs, const uint32_t* srcSizes, uint32_t maxChunk,
                                           uint32_t nChunks, uint8_t* const* dstPtrs, const uint32_t* dstCaps,
                                           int32_t* outSizes, const uint8_t* const* dictPtrs,
                                           const uint32_t* dictSizes, uint32_t nDicts, const uint8_t* states,
                                           const uint32_t* chunkDict, int level, uint8_t* ws, uint32_t slots,
                                           hipStream_t st);
// -BD at level >= 3: segments [begin[k], end[k]) of src (begin >= -64 KiB),
// blockSeg[b] = block b's segment; delta0 = chain scratch for src[0], with
// 64 Ki entries before it.
hipError_t launch_encode_hc_bd(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                               uint8_t* slots, const int64_t* segBegin, const int64_t* segEnd, uint32_t nSeg,
                               const uint32_t* blockSeg, uint16_t* delta0, int32_t* csize, hipStream_t st);
hipError_t launch_encode_linked(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                                uint8_t* slots, const LinkPlan* plan, uint32_t* table, bool fresh, bool xh, int32_t* csize,
                                hipStream_t st);
// The block-dependent encode as parallel fixed-point rounds
// (k_encode_linked_round / k_link_settle; the serial kernel finishes from
// the first unsettled block if kLinkRounds rounds do not settle).
constexpr int kLinkRounds = 32;
uint64_t link_round_bytes(uint64_t nBlocks);   // scratch: entry + exit tables, round control words
hipError_t launch_encode_linked_par(const uint8_t* src, uint64_t srcSize, uint32_t blockSize, uint32_t nBlocks,
                                    uint8_t* slots, const LinkPlan* plan, uint32_t* table, bool fresh, bool xh,
                                    uint32_t* scratch, int32_t* csize, int rounds, hipStream_t st);
hipError_t launch_decode_linked(const uint8_t* frame, const BlockRec* recs, uint32_t nBlocks, uint32_t blockMax,
                                uint8_t* out, uint64_t outCap, uint8_t* slot, uint8_t* hist, const uint32_t* digest,
                                int blockChecksum, int32_t* dsize, int32_t* status, hipStream_t st);
// The same contract as launch_decode_linked (status, dsize, out, hist in/out),
// decoded in parallel fixed-point rounds (k_dlink_*; serial finish if
// `rounds` do not settle).  scratch: dlink_scratch_bytes(nBlocks, blockMax).
uint64_t dlink_scratch_bytes(uint64_t nBlocks, uint32_t blockMax);
// LZ4MT_AMD_BD_ROUNDS=k caps the -BD encode's parallel rounds (tests: the
// serial finish from the first unsettled block); default kLinkRounds
inline int env_rounds() {
    const char* e = getenv("LZ4MT_AMD_BD_ROUNDS");
    return e ? atoi(e) : kLinkRounds;
}
// LZ4MT_AMD_BD_REFERENCE=1: -BD frames with 1 and 4 MiB blocks written byte
// for byte as the reference writes them (its input buffer replayed by BdSim:
// each block after the first read over its own dictionary, frames that do
// not decode back -- DESIGN.md §1).  Off by default: the decodable stream.
inline bool bd_reference_bytes() {
    const char* e = getenv("LZ4MT_AMD_BD_REFERENCE");
    return e && e[0] == '1';
}
// LZ4MT_AMD_BD_SERIAL=1: the one-wave -BD kernels only (A/B and tests)
inline bool bd_serial() {
    const char* e = getenv("LZ4MT_AMD_BD_SERIAL");
    return e && e[0] == '1';
}
hipError_t launch_decode_linked_par(const uint8_t* frame, const BlockRec* recs, uint32_t nBlocks, uint32_t blockMax,
                                    uint8_t* out, uint64_t outCap, uint8_t* hist, const uint32_t* digest,
                                    int blockChecksum, int32_t* dsize, int32_t* status, uint8_t* scratch, int rounds,
                                    hipStream_t st);

}  // namespace lz4mt
