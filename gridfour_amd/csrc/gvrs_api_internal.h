// gvrs_api_internal.h -- what the translation units of the C ABI (gvrs_api*.hip) share: the context, its buffers and lock, the
// error helpers and the functions that cross files.  Host code only: no kernel source includes it.  Nothing declared here is an
// export of the library (hidden visibility); what a file keeps to itself stays static there.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <sched.h>
#include <zlib.h>

#include "../../include/gvrs_hip_codec.h"
#include "gvrs_kernels.h"
#include "gvrs_encode_layout.h"
#include "gvrs_carve.h"
#include "gvrs_lsop_container.h"
#include "gvrs_file_parse.h"
#include "gvrs_stage.h"

#pragma GCC visibility push(hidden)

extern thread_local std::string g_lastError;   // (gvrs_api.hip: gf_last_error)
#ifdef GF_DIAG
// the diagnostic flavour of the library only (libgvrs_hip_diag.so, tools/): process-wide hooks for phase ablation and
// the kernels' cycle stamps.  The shipping library has no mutable global state.
extern int g_encPhaseLimit, g_decPhaseLimit;
extern uint32_t *g_decodeDebug;   // 16 cycle stamps per tile
extern uint32_t *g_encodeDebug;   // dump target of the next encode launches
#else
constexpr int g_encPhaseLimit = 0, g_decPhaseLimit = 0;
constexpr uint32_t *g_decodeDebug = nullptr, *g_encodeDebug = nullptr;
#endif

inline gf_status hipFail(hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    g_lastError = buf;
    return GF_ERR_HIP;
}

#define GF_HIP(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hipFail(e_, #call); \
    } while (0)

// offsets[nTiles + 1] of a caller's blob: non-decreasing, every packing shorter than 4 GiB (lengths travel as uint32)
inline bool offsetsValid(const uint64_t *offsets, size_t nTiles)
{
    for (size_t t = 0; t < nTiles; t++)
        if (offsets[t + 1] < offsets[t] || offsets[t + 1] - offsets[t] > 0xFFFFFFFFull) return false;
    return true;
}

// Counts the device buffers that moved (a move is rare: buffers only grow).  A recorded hipGraph holds the addresses it was
// captured with: the one-tile graphs (gf_single) remember the count they were recorded at and are dropped when it has changed.
// A context's buffers count on the CONTEXT's counter (gf_context::bufMoves): another GPU's shard or another thread's batch must
// not make every context re-record its graphs.  This one is for the buffers that belong to no context.
inline std::atomic<uint64_t> g_devBufMoves{0};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    std::atomic<uint64_t> *moves = &g_devBufMoves;
    DevBuf *next = nullptr;                         // the owner's list (gf_context::bufs)
    bool staged = false;                            // a host form's Stage is live in it (gvrs_stage.h)
    DevBuf() = default;
    explicit DevBuf(gf_context *owner);             // a context's buffer: links itself in and counts on the context's counter
    DevBuf(const DevBuf &) = delete;
    // a laid-out buffer: the Carve's parts + slack bytes; at<T>(offset) is a part
    gf_status ensure(const Carve &k, size_t slack = 16) { return ensure(k.total + slack); }
    template <class T> T *at(size_t offset) const { return (T *)((uint8_t *)p + offset); }
    gf_status ensure(size_t need)
    {
        if (need <= bytes) return GF_OK;
        moves->fetch_add(1, std::memory_order_relaxed);
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        need = roundUp(need + need / 8, 1 << 20);
        GF_HIP(hipMalloc(&p, need));
        bytes = need;
        return GF_OK;
    }
    void release()
    {
        if (p) {
            moves->fetch_add(1, std::memory_order_relaxed);
            (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
    }
};

// page-locked host memory that grows on demand (the staging slots of gvrs_api_host.hip)
struct PinBuf {
    void *p = nullptr;
    size_t bytes = 0;
    gf_status ensure(const Carve &k, size_t slack = 0) { return ensure(k.total + slack); }
    template <class T> T *at(size_t offset) const { return (T *)((uint8_t *)p + offset); }
    gf_status ensure(size_t need)
    {
        if (need <= bytes) return GF_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        need = roundUp(need + need / 8, 1 << 20);
        GF_HIP(hipHostMalloc(&p, need, hipHostMallocDefault));
        bytes = need;
        return GF_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// A DevBuf is one line here: it links itself into bufs.
struct gf_context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::atomic<uint64_t> bufMoves{0};          // moves of THIS context's device buffers (DevBuf::moves): what its recorded graphs watch
    DevBuf *bufs = nullptr;                     // every DevBuf below (declared before them: they link themselves in)
    // scratch of the device forms, laid out by scratchPlan and sized ahead by gf_context_reserve
    DevBuf workspace{this};      // decode spill: grid * 6*cells
    DevBuf trees{this};          // leaf records of the tree pre-pass: GF_TREE_REC_WORDS per tile
    DevBuf packRecs{this};       // encoder: selection records between k_huffman_encode and k_huffman_pack
    DevBuf flags{this};          // one word: tiles the fast decode kernel left to the general one (GfDecodeArgs::retryFlag)
    DevBuf dStage{this};         // the staging of the host-memory entry points: one Stage at a time (HostStage below)
    DevBuf dValues{this}, dStatus{this}, dM32{this}, dM32Len{this}, dM32Models{this}, dSeeds{this};   // CodecDeflate's host encoder: a chunk's tiles,
                                                // statuses and candidate streams (deflateEncodeBatchHost, which overlaps its chunks)
    DevBuf dResiduals{this}, dCoefs{this}, dStatus2{this};   // LSOP12 under the records driver: residuals, coefficients, the second status
    DevBuf dInflate{this}, dInflOut{this}, dInflMeta{this};  // GPU inflate: stream descriptors, inflated bytes, produced / status
    DevBuf dBlockTmp{this}, dBlockIdx{this}, dBlockSlots{this};   // grid blocks (gvrs_api_blocks.hip): the records' decoded tiles on their way into a block,
                                                // the gather's element table and the records' tile indices, the slot table of the block's tiles
    DevBuf dRecMeta{this}, dRecSub{this}, dRecTmp{this};          // records / mixed packings in device memory (gvrs_api_records_dev.hip): per-record framing
                                                // results, the partition by codec, decoded tiles on their way to their place
    DevBuf dBwTiles{this}, dBwMeta{this};       // a block written (gvrs_api_blocks_write.hip): the elements' cut tiles, the tiles' flags and pre-status;
                                                // a file written at points (gvrs_api_file_points.hip): the elements' owner planes, the slots' old
                                                // status, stored flag and pre-status (its pool lies in dBlockTmp, its records in dFileUpdateBlob)
    DevBuf dEncSlots{this}, dEncMeta{this}, dEncWide{this};       // records written in device memory (gvrs_api_records_enc.hip): the codecs' candidate slots,
                                                // their lengths / statuses and the records' layout, SHORT cells widened for the codecs
    DevBuf dDsBlocks{this};                     // downsampling (gvrs_api_downsample.hip): the record forms' full-resolution blocks
    DevBuf dImage{this};                        // images (gvrs_api_image.hip): the record forms' three planes
    DevBuf dTabPartials{this}, dTabSort{this};  // tabulation (gvrs_api_tabulate.hip): k_tabulate_dense's partials (fixed size); the symbol form's
                                                // keys, histograms and runs, a strip's table and the merge's chunk counts
    DevBuf dFileLoc{this};                      // file images (gvrs_api_file.hip): the extents and verdicts of the rectangle's tiles
    DevBuf dFilePoints{this};                   // file images read at points (gvrs_api_file_points.hip): the bitmap of touched tiles, its prefixes,
                                                // the list with its extents and verdicts, the slots' statuses; the pool itself lies in dBlockTmp
    DevBuf dFileWrite{this};                    // file images written (gvrs_api_file_write.hip): the kernels' state, the records' offsets, the
                                                // metadata directory on its way to its place, the tile directory's chunk checksums
    DevBuf dFileUpdateBlob{this};               // ... the records of a rectangle on their way into the image, and their offsets
    DevBuf dFileUpdate{this};                   // file images updated (gvrs_api_file_update.hip): state, positions, the free list, the old entries
    DevBuf dFileInspect{this};                  // file images inspected (gvrs_api_file_inspect.hip): state, the segments' anchors and walks, the record list
    DevBuf dTabBlocks{this};                   // ... the composed read's blocks (gf_block_read_tabulated_symbols_elems[_dev])
    // Every entry point that takes the context holds this lock for its duration (GF_CTX_LOCK): the reference calls ONE decoder
    // instance from several threads (gvrs/RasterTileCache.java:418-421, TileDecompressionAssistant.java:68-73), and a context's
    // scratch buffers, staging slots and recorded graphs are one set.  Recursive: entry points call each other.
    std::recursive_mutex mu;
    GfSideStream side{nullptr, nullptr, nullptr};   // second stream + fork / join events: the fast decode kernel's roomy run (gvrs_kernels.h)
    uint32_t *hRoomySeen = nullptr;                 // page-locked word: GfDecodeArgs::roomySeenHost
    PinBuf hRecCounts;                              // page-locked: the partition's counts on their way to the host
    PinBuf hFileFront;                              // page-locked: a written file's header, metadata records and metadata directory on their
    hipEvent_t fileFrontDone = nullptr;             // way to the device; recorded behind their copies (gvrs_api_file_write.hip)
    // what the last encode and the last decode batch launched (host side only: gf_internal_route_report)
    uint32_t routeEnc = 0, routeDec = 0;            // GF_RT_* bits
    int routeEncKind = -1, routeDecKind = -1, routeRoomy = GF_ROOMY_NONE, routePrepass = 0;
    struct gf_host_pipe *pipe = nullptr;        // pipelined staging of the host-memory batch entry points (created on first use)
    struct gf_single *single = nullptr;         // one tile per call: page-locked buffers and replayed graphs (created on first use)
};
void gf_host_pipe_destroy(struct gf_host_pipe *p);   // (gvrs_api_host.hip, as the next)
void gf_single_destroy(struct gf_single *s);
inline DevBuf::DevBuf(gf_context *owner) : moves(&owner->bufMoves), next(owner->bufs) { owner->bufs = this; }
#define GF_CTX_LOCK(c)                                       \
    std::unique_lock<std::recursive_mutex> gfCtxLock_;       \
    if (c) gfCtxLock_ = std::unique_lock<std::recursive_mutex>((c)->mu)

// The staging of a host form (gvrs_stage.h) in the context's dStage, on the context's stream.  One stage at a time: a host form that
// began one ends it before it calls another host form, and begin() on a buffer in use fails the call (GF_ERR_HIP, gf_last_error).
struct StageDev {
    typedef gf_status Status;
    DevBuf &buf;
    hipStream_t st;
    bool &busy() { return buf.staged; }
    gf_status reserve(size_t bytes, unsigned char *&base) { const gf_status s = buf.ensure(bytes + 16); base = (unsigned char *)buf.p; return s; }
    gf_status toDevice(void *d, const void *h, size_t n) { GF_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st)); return GF_OK; }
    gf_status toHost(void *h, const void *d, size_t n) { GF_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, st)); return GF_OK; }
    gf_status zero(void *d, size_t n) { GF_HIP(hipMemsetAsync(d, 0, n, st)); return GF_OK; }
    gf_status sync() { GF_HIP(hipStreamSynchronize(st)); return GF_OK; }
    gf_status refuse(const char *why) { g_lastError = why; return GF_ERR_HIP; }
};
struct HostStage : Stage<StageDev> {
    explicit HostStage(gf_context *c) : Stage<StageDev>(StageDev{c->dStage, c->stream}) {}
};
static_assert(STAGE_MAX_PARTS >= 2 * GF_MAX_ELEMS + 12, "a stage holds every element's array twice and a dozen single parts");

// the caller's stream, or the context's own
inline hipStream_t streamOf(const gf_context *c, void *stream) { return stream ? (hipStream_t)stream : c->stream; }

// codec kinds behind the shared batch plumbing
enum { KIND_HUFFMAN = 0, KIND_CANON = 1, KIND_RAW_M32 = 2, KIND_DEFLATE = 3, KIND_FLOAT = 4 };

// ---- the scratch plan (gvrs_api_route.hip): what a batch of a kind needs of workspace, trees and packRecs, and where the parts lie.
// The launch sites take sizes and offsets from it and gf_context_reserve allocates its maximum over the kinds: no _dev call after it allocates.
enum { KIND_LSOP_DEC = 5, KIND_LSOP_ENC = 6 };      // LSOP12's needs, beside the KIND_* of the route plan
struct gf_scratch_part { uint64_t at, bytes; };
struct gf_scratch_plan {
    uint64_t workspace, trees, packRecs;            // bytes needed
    uint64_t wsStride, planeStride;                 // bytes per workgroup of the decode grid in workspace, per tile of the byte plane (0: none)
    gf_scratch_part leaf, spare, roomy;             // trees, CodecHuffman decode: leaf records, four spare words, the roomy run's tile list
    gf_scratch_part lengths, slack;                 // trees, CodecCanonHuffman decode: length records, the slack behind them (the fast run's where viaFast)
    gf_scratch_part lsop0, lsop1;                   // trees, LSOP12 decode: the length records of the two streams
    gf_scratch_part sel, stats, plane, hist;        // packRecs: selection records, statistics, byte plane (not lean); LSOP12 encode: histogram records
};
gf_status scratchPlan(int kind, int nRows, int nCols, size_t nTiles, int lean, int viaFast, gf_scratch_plan &p);
void scratchReserve(int nRows, int nCols, size_t nTiles, uint64_t need[3]);       // workspace, trees, packRecs: the maximum over the kinds

constexpr size_t INFLATE_SCRATCH_BYTES = (size_t)1 << 30;     // thousands of streams per launch: a stream is one serial chain

unsigned hostCores();   // (gvrs_api.hip)

// tiles are independent: the host-side zlib stages run on every core the process may use
template <class F>
static void parallelFor(size_t n, F f)
{
    unsigned nt = hostCores();
    if (nt > n) nt = (unsigned)n;
    if (nt == 1) { for (size_t i = 0; i < n; i++) f(i); return; }
    std::vector<std::thread> th;
    for (unsigned w = 0; w < nt; w++)
        th.emplace_back([=]() { for (size_t i = w; i < n; i += nt) f(i); });
    for (auto &x : th) x.join();
}

// (putLE32, roundUp and zDeflate: gvrs_lsop_container.h)
inline uint32_t getLE32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// One tile through a codec's batch entry point (the ICompressionEncoder / ICompressionDecoder form): batch(offsets, &tileStatus) is
// that call for one tile.  *outLen is written even when it fails; the tile's status replaces GF_OK only.
template <class Batch>
static gf_status oneTileEncode(size_t *outLen, Batch batch)
{
    if (!outLen) return GF_ERR_ARG;
    uint64_t offsets[2] = {0, 0};
    int32_t st = 0;
    const gf_status s = batch(offsets, &st);
    *outLen = (size_t)offsets[1];
    return s != GF_OK ? s : (gf_status)st;
}
template <class Batch>
static gf_status oneTileDecode(size_t len, Batch batch)
{
    uint64_t offsets[2] = {0, (uint64_t)len};
    int32_t st = 0;
    const gf_status s = batch(offsets, &st);
    return s != GF_OK ? s : (gf_status)st;
}

// ---- the functions that cross files.  lean: 1 from the one-tile-per-call path alone (GfEncodeArgs::lean, GfDecodeArgs::lean)
// gvrs_api_route.hip
gf_status encodeBatchDev(int kind, gf_context *c, void *stream, int codecIndex, int nRows, int nCols, size_t nTiles,
                         const int32_t *dValues, uint8_t *dOut, size_t slotStride, uint32_t *dLengths, uint8_t *dPredictors,
                         int32_t *dStatus, int predictorMask, int lean);
gf_status decodeBatchDev(int kind, gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                         size_t blobBytes, const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues,
                         int32_t *dStatus, int lean, uint32_t *analysis = nullptr, uint32_t *pairCounts = nullptr);
// gvrs_api_host.hip
gf_status decodeBatchHostG(int kind, gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                           const uint64_t *starts, const uint32_t *lens, const uint32_t *dstTile, int32_t *values, int32_t *status);
gf_status decodeBatchHost(int kind, gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                          int32_t *values, int32_t *status);
// gvrs_api_float.hip
gf_status floatDecodeDev(gf_context *c, hipStream_t st, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                         const uint64_t *dOffsets, const uint32_t *dLengths, float *dValues, int32_t *dStatus);
bool zDeflateUpTo(const uint8_t *in, size_t n, int level, size_t limit, std::vector<uint8_t> &out);
// gvrs_api_records_dev.hip: the argument checks of the elements calls, an element's bytes per cell, and the one device pipeline
// (no lock taken, no argument checked: its callers hold the context's lock)
gf_status elemsArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                    size_t nTiles, const uint8_t *blob, bool blobOnDevice, const uint64_t *offsets, void *const *values,
                    const int32_t *status);
size_t elemItemBytes(int type);
// one array of `count` cells per element (+ slack bytes behind each) as parts of a stage: element e's lies at host[e], part[e] is its number
inline void stageElems(HostStage &sg, unsigned flags, const gf_elem_spec *elems, int nElems, size_t count, const void *const *host, int *part,
                       size_t slack = 0)
{
    for (int e = 0; e < nElems; e++) part[e] = sg.add(const_cast<void *>(host[e]), count * elemItemBytes(elems[e].type), flags, slack);
}
// ... and in a buffer that holds those arrays alone: ensured, arrays[e] is element e's
inline gf_status elemArrays(DevBuf &b, const gf_elem_spec *elems, int nElems, size_t count, void **arrays, size_t extra = 0)
{
    Carve k;
    size_t item[GF_MAX_ELEMS], at[GF_MAX_ELEMS];
    for (int e = 0; e < nElems; e++) item[e] = elemItemBytes(elems[e].type);
    k.each(nElems, count, item, at, extra);
    const gf_status s = b.ensure(k);
    for (int e = 0; e < nElems && s == GF_OK; e++) arrays[e] = b.at<void>(at[e]);
    return s;
}
gf_status recordsDecodeDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows,
                           int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                           const uint32_t *dLengths, int verifyChecksum, int32_t *dTileIndices, void *const *dValues, int32_t *dStatus,
                           const uint64_t *dEnds = nullptr);
// gvrs_api_records_enc.hip: the argument checks of the record writer, "this list needs nothing from the host", the one device
// pipeline (dPreStatus, may be null: per tile a non-zero status that replaces the record) and the host encoders' path
gf_status encArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                  size_t nTiles, const int32_t *tileIndices, const void *const *values, const uint8_t *blob, size_t blobCap,
                  const uint64_t *offsets, bool onDevice, const int32_t *dStatus);
bool deviceList(const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems);
gf_status recordsEncodeDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows,
                           int nCols, size_t nTiles, const int32_t *dTileIndices, const void *const *dValues, int checksumEnabled,
                           uint8_t *dBlob, size_t blobCap, uint64_t *dOffsets, uint8_t *dCodecUsed, int32_t *dStatus,
                           const int32_t *dPreStatus = nullptr);
gf_status recordsEncodeHost(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                            size_t nTiles, const int32_t *tileIndices, const void *const *values, int checksumEnabled, uint8_t *blob,
                            size_t blobCap, uint64_t *offsets, uint8_t *codecUsed);
// gvrs_api_blocks.hip: the geometry of a block call (what the host can check; fills g), ARG before UNSUPPORTED, the fills' bits
gf_status blockGeom(const gf_grid_spec *grid, const gf_rect *rect, GfBlockGeom &g);
gf_status firstOf(gf_status a, gf_status b);
gf_status elemFills(const gf_elem_spec *elems, int nElems, uint32_t *fill);
// ... a block read's argument checks (fills g and fill), and records in device memory -> one block per element in device memory
// (no lock taken, no argument checked)
gf_status blockReadArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const gf_grid_spec *grid,
                        const gf_rect *rect, size_t nRecords, const uint8_t *blob, bool blobOnDevice, const uint64_t *offsets,
                        void *const *blocks, const int32_t *status, GfBlockGeom &g, uint32_t *fill);
gf_status blockReadDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const GfBlockGeom &g,
                       const uint32_t *fill, size_t n, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets, int verifyChecksum,
                       void *const *dBlocks, int32_t *dStatus, const uint64_t *dEnds = nullptr, const int32_t *dVerdict = nullptr);
// gvrs_api_blocks_write.hip: a block write's argument checks (fills g and the cut's element descriptions), and blocks in device
// memory -> records in device memory (no lock taken, no argument checked)
gf_status blockWriteArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, const gf_elem_range *ranges, int nElems,
                         const gf_grid_spec *grid, const gf_rect *rect, const void *const *blocks, size_t nOld, const uint8_t *oldBlob,
                         const uint64_t *oldOffsets, const uint8_t *blob, size_t blobCap, const uint64_t *offsets, const int32_t *tileIndices,
                         const int32_t *status, bool onDevice, GfBlockGeom &g, GfBlockCutElem *cut);
gf_status blockWriteDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const GfBlockGeom &g,
                        const GfBlockCutElem *cut, const void *const *dBlocks, size_t nOld, const uint8_t *dOldBlob, size_t oldBlobBytes,
                        const uint64_t *dOldOffsets, int verifyOldChecksum, int checksumEnabled, uint8_t *dBlob, size_t blobCap, uint64_t *dOffsets,
                        int32_t *dTileIndices, uint8_t *dCodecUsed, int32_t *dStatus, const uint64_t *dOldEnds = nullptr);
// ... the cut's description of every element (block, tiles and old tiles are left null); ranges == null: the default ranges
gf_status cutElems(const gf_elem_spec *elems, const gf_elem_range *ranges, int nElems, GfBlockCutElem *t);
// ... and the tail of a host form that writes records: the nOut tiles dTiles of the device, with the pre-status dPre, to records
// in HOST memory.  sg is the call's begun stage and holds the parts named here (indices: out; blob: held, maxBlob bytes; offsets,
// status, used: out, declared with their host places for a device list and with null otherwise); the tail ends the stage.  A
// device list goes through recordsEncodeDev, any other brings tiles and verdicts back and goes through recordsEncodeHost.
struct HostWriteParts { int indices, blob, offsets, status, used; };
gf_status hostWriteTail(gf_context *c, HostStage &sg, const HostWriteParts &p, bool onDevice, const int *codecs, int nCodecs, const gf_elem_spec *elems,
                        int nElems, int nRowsTile, int nColsTile, size_t nOut, const void *const *dTiles, const int32_t *dPre, int checksumEnabled,
                        size_t maxBlob, uint8_t *blob, size_t blobCap, uint64_t *offsets, int32_t *tileIndices, uint8_t *codecUsed, int32_t *status);
// gvrs_api_file_update.hip: the handle's content, and the records form behind its null checks (the caller holds the lock)
struct GfFileUpdate;
const GfFileUpdate &fileUpdateOf(const gf_file_update *u);
gf_status updateRecordsDev(gf_context *c, const GfFileUpdate &h, uint8_t *dImage, size_t imageCap, const uint8_t *dBlob, const uint64_t *dOffsets,
                           const int32_t *dTileIndices, const int32_t *dStatus, int32_t *dTileStatus, size_t nRecords, size_t blobBytes,
                           int64_t timeModified, int flags, size_t listCapacity, uint64_t *dImageBytes, int32_t *dFileStatus);
// gvrs_api_file.hip: k_file_locate for the rectangle's tiles on a stream (no lock taken): a.starts, a.ends, a.verdict lie in dFileLoc
gf_status fileLocateDev(gf_context *c, hipStream_t st, const gf_file_info &i, const uint8_t *dImage, size_t imageBytes, const GfBlockGeom &g,
                        uint8_t *dPresent, GfFileLocateArgs &a);
// gvrs_api_file_write.hip: host bytes to device memory through the context's page-locked hFileFront, enqueued like the kernels
struct FileFrontPart { const void *host; void *dev; size_t bytes; };   // (0 bytes: nothing travels)
gf_status fileFrontSend(gf_context *c, hipStream_t st, std::initializer_list<FileFrontPart> parts);
// the largest tile record of a file with these elements and tiles, refused where its size does not travel as an int32
inline gf_status fileMaxRecord(const gf_elem_spec *elems, int nElems, const GfBlockGeom &g, size_t &maxRecord)
{
    maxRecord = gf_tile_record_max_bytes_elems(elems, nElems, g.nRowsTile, g.nColsTile);
    return maxRecord == 0 || maxRecord > 0x7fffffffull ? GF_ERR_UNSUPPORTED : GF_OK;
}
// gvrs_api_interp.hip: what the host can check of an interpolation spec (fills g)
gf_status interpSpecArgs(const gf_context *c, const gf_interp_spec *spec, const void *block, bool perPointSpacing, GfInterpGeom &g);
// gvrs_api_coords.hip: the coordinate facts of a file as the rules of gvrs_coords.h take them, with what the reference derives;
// and the answer to a NULL context behind every other argument check: GF_ERR_NO_DEVICE on a machine without a device (no
// context can be had there), GF_ERR_ARG otherwise
GfCoords coordsOf(const gf_file_info &i);
gf_status noContext();
// gvrs_api_records.hip
size_t elemStandardSize(int elemType, size_t cells);
// gvrs_api_lsop.hip: gf_lsop08_decode_batch_i32_dev on a stream (the public form runs on the context's own)
gf_status lsop08DecodeDev(gf_context *c, hipStream_t st, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                          const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus,
                          int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus);
// gvrs_api_deflate.hip
gf_status deflateDecodeDev(gf_context *c, hipStream_t st, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                           const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus);
gf_status codecMasterDecodeScattered(gf_context *c, const int *codecs, int nCodecs, int nRows, int nCols, size_t nTiles,
                                     const uint8_t *blob, const uint64_t *starts, const uint32_t *lens, const uint8_t *skip,
                                     int32_t *values, int32_t *st);

#pragma GCC visibility pop
