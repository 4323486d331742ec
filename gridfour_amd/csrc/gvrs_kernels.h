// gvrs_kernels.h -- launch interface between the C ABI (gvrs_api.hip) and the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "gvrs_interp_common.h"
#include "gvrs_render_common.h"
#include "gvrs_downsample_common.h"
#include "gvrs_image_common.h"
#include "gvrs_tabulate_common.h"
#include "gvrs_lsop_container.h"
#include "gvrs_file_parse.h"
#include "gvrs_file_points.h"
#include "gvrs_coords.h"

// per-tile status values written by the kernels; identical to gf_status in
// include/gvrs_hip_codec.h
#define GF_K_OK 0
#define GF_K_DECLINED 1
#define GF_K_OVERFLOW 2
#define GF_K_ERR_FORMAT (-1)
#define GF_K_ERR_BOUNDS (-2)
#define GF_K_ERR_ARG (-4)
#define GF_K_ERR_UNSUPPORTED (-7)

// One tile per workgroup and NO tile loop in the kernel.  A persistent grid-stride loop over tiles invites the compiler to hoist
// every thread-index and tile-shape term out of it; at the kernels' register caps those dozens of hoisted values are then
// spilled (VGPRs to scratch -- stored and reloaded once per tile, i.e. HBM traffic; SGPRs into lanes of reserved VGPRs).
// Measured on the bench batch: k_huffman_decode<fast> 118 -> 86 VGPRs, 72 -> 11 spilled SGPRs, 1.43 -> 1.31 ms;
// k_huffman_pack 14 -> 6 spilled VGPRs.  GF_FOR_WG_TILE is a `for` that runs at most once (so `continue` / `break` keep
// their meaning); gf_tile_grid spreads the tiles over x and y so that any tile count fits one launch.
#define GF_FOR_WG_TILE(t, nTiles) \
    for (size_t t = (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x; t < (size_t)(nTiles); t = ~(size_t)0)
// the same with the choice left to a template parameter: a persistent grid-stride loop (1-D grid) when ONESHOT is false
#define GF_FOR_TILES(t, nTiles, ONESHOT) \
    for (size_t t = (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x; t < (size_t)(nTiles); t = (ONESHOT) ? ~(size_t)0 : t + gridDim.x)
inline dim3 gf_tile_grid(size_t nTiles)
{
    const size_t gx = nTiles < (1u << 20) ? (nTiles ? nTiles : 1) : (1u << 20), gy = (nTiles + gx - 1) / gx;
    return dim3((unsigned)gx, (unsigned)(gy ? gy : 1), 1);
}

// The pre-pass kernels (k_huffman_parse_trees, k_canon_parse_lengths) walk one tile per LANE: a serial walk of some hundred
// steps per tile.  A large batch fills the chip that way (12,960 tiles = 203 waves, and every wave instruction serves 64
// tiles); a small one does not -- 1,024 tiles are 16 waves on 1,024 SIMDs, each crawling through the divergent walks of 64
// trees.  Small batches therefore give every tile a wave of its own -- an instantiation with ONE active lane, which the compiler
// turns into scalar code (with 2 or 4 lanes, or the lane count as a kernel argument, half the gain is lost): decode of the
// 1,024-tile batch 0.339 -> 0.300 ms; on the 12,960-tile batch the same costs 0.07 ms, 16 or 8 tiles per wave 0.01-0.02 ms.
#ifndef GF_PREPASS_ONE_LANE_MAX
#define GF_PREPASS_ONE_LANE_MAX 4096      // 120x150 tiles, decode ms with a lane / a wave per tile: 2,048 tiles 0.308 / 0.280, 3,000
                                          // 0.403 / 0.386, 4,096 0.511 / 0.502, 6,000 0.703 / 0.710, 8,192 0.904 / 0.920
#endif
inline unsigned gf_prepass_tiles_per_wave(size_t nTiles) { return nTiles <= GF_PREPASS_ONE_LANE_MAX ? 1u : 64u; }

// Dynamic LDS beyond the default limit must be opted into, per kernel and PER DEVICE (hipFuncSetAttribute acts on the
// current device's copy of the function).  One GfDynLdsOptIn per kernel remembers the largest size asked for on each
// device; contexts on different devices and threads of one process share it safely.
constexpr int GF_MAX_DEVICES = 64;
struct GfDynLdsOptIn {
    size_t done[GF_MAX_DEVICES] = {};
    std::mutex mu;
};
template <class K>
inline hipError_t gf_opt_in_dyn_lds(K kernel, size_t dyn, GfDynLdsOptIn &st)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= GF_MAX_DEVICES) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(st.mu);
    if (dyn <= st.done[dev]) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e == hipSuccess) st.done[dev] = dyn;
    return e;
}

struct GfEncodeArgs {
    const int32_t *values;     // nTiles * nRows*nCols
    uint8_t *out;              // nTiles slots of slotStride bytes
    uint32_t *lengths;
    uint8_t *predictors;       // may be null
    int32_t *status;
    size_t nTiles;
    size_t slotStride;
    int nRows, nCols;
    int codecIndex;
    int predictorMask;
    uint32_t *debug;           // optional diagnostic dump (GF_ENC_DEBUG_WORDS per tile), normally null
    int phaseLimit;            // diagnostic: stop after phase A (1) / B (2); 0 = run everything
    uint32_t *retryFlag;       // CodecHuffman: two device words (the second one counts the tiles k_huffman_pack leaves to k_huffman_pack_rare; no kernel sets the
                               // first: the fast encode kernel leaves no tile to the general one); null: general kernel only
    uint32_t *packRecs;        // non-null (CodecHuffman only): k_huffman_encode stops after the selection and leaves per tile
                               // GF_PACK_REC_WORDS words (model, tree end bit, seed, maxN, maxLen, tree image, code table)
                               // for k_huffman_pack, which writes the packing
    int lean;                  // 1 (the one-tile-per-call path): only the kernels a tile usually needs are launched; a tile that
                               // needs another one (k_huffman_pack_rare) is reported with the internal status GF_K_LEAN_RETRY and
                               // the caller takes the batch path for it
    uint32_t *encStats;        // non-null (CodecHuffman batches): the encoder runs as k_huffman_encode (histograms only) +
                               // k_huffman_trees (one wave per tile); GF_ENC_STAT_WORDS words per tile between them
    uint8_t *plane;            // non-null (CodecHuffman batches with encStats, round 6): phase A leaves every cell's RAW ROW DIFFERENCE
                               // as one byte -- v - W, column 0: v - N, the seed cell 0 -- at plane + t * planeStride + cell, and marks
                               // the tile (word 8 of its statistics record) when every one of them is that byte exactly; the packer
                               // then derives the winner's residuals from the plane (1 byte per cell) instead of reading the tile again
    size_t planeStride;        // bytes per tile: the cells rounded up to a multiple of 16
};
constexpr int GF_ENC_STAT_WORDS = 16 + 3 * 256;   // models, seed, longest value per predictor, a "has work" mark; the three histograms
#define GF_K_LEAN_RETRY 0x7fff0002              /* (= GF_K_RETRY of the kernels: the fast kernels' own mark travels the same way) */
constexpr int GF_PACK_REC_WORDS = 8 + 88 + 512;

struct GfDecodeArgs {
    const uint8_t *blob;       // 4-byte aligned
    size_t blobBytes;
    const uint64_t *offsets;   // may be null -> t * slotStride
    size_t slotStride;
    const uint32_t *lengths;
    int32_t *values;
    int32_t *status;
    uint8_t *workspace;        // gridDim.x * workspaceStride bytes (M32 spill)
    size_t workspaceStride;
    size_t nTiles;
    int nRows, nCols;
    uint32_t ldsM32Bytes;      // capacity of the in-LDS M32 buffer
    uint32_t ldsTextBytes;     // capacity of the in-LDS copy of the packing (multiple of 16)
    uint32_t ldsStageBytes;    // k_canon_decode: bytes of value staging behind the text copy (gf_canon_decode_lds_stage)
    int phaseLimit;            // diagnostic: stop after phase 0/1/2 (value 1/2/3); 0 = run everything
    uint32_t *debug;           // diagnostic: 16 cycle stamps per tile, normally null
    int rawM32;                // 1: the container holds the M32 bytes themselves behind the 10-byte header (CodecDeflate after inflate)
    const uint32_t *trees;     // non-null: the Huffman trees were parsed by k_huffman_parse_trees (GF_TREE_REC_WORDS per tile)
    uint32_t *retryFlag;       // non-null (CodecHuffman batches with tree records): two device words; the fast kernel ORs 1 into
                               // word (ldsM32Roomy ? 1 : 0) for every tile it leaves to the general kernel (status GF_K_RETRY
                               // inside the launch only), which looks at that word.  With ldsM32Roomy the fast kernel runs twice,
                               // each run taking the tiles the pre-pass gave it (GF_TREE_ROOMY in the tile's tree record)
    uint32_t ldsM32Roomy;      // 0, or the M32 capacity of the fast kernel's second run (round 4): tiles whose M32 stream or
                               // packing outgrows ldsM32Bytes (dense in multi-byte values) get a workgroup with more LDS
                               // instead of the general kernel and its workspace in global memory
    const uint32_t *roomyList; // the tiles of the roomy run, listed by the pre-pass; retryFlag[2] = their count, retryFlag[3] = the
                               // cursor the run's workgroups draw from (both zeroed again by the general kernel, the batch's last)
    uint32_t *roomySeenHost;   // may be null: a word of page-locked host memory that receives 1 + that count from the general kernel --
                               // the host's hint for the NEXT batch (does the roomy run have work, i.e. is it worth a second stream?)
    int flagsCleared;          // 1: the tree pre-pass zeroed retryFlag (gf_launch_huffman_parse_trees), no memset in front of the kernels
    int lean;                  // 1 (the one-tile-per-call path): the fast kernel alone; what it leaves behind keeps the status
                               // GF_K_LEAN_RETRY and the caller takes the batch path for it
    uint32_t *analysis;        // non-null: CodecHuffman.analyze mode -- per tile GF_ANALYSIS_WORDS words (predictor, nM32,
                               // bits in tree, packing bytes - 10, 256-bin histogram of the M32 bytes); no values are written.
                               // CodecCanonHuffman batches: GF_CANON_STAT_WORDS words per tile from k_canon_stats (gf_launch_canon_analyze)
    uint32_t *pairCounts;      // analyze mode, may be null: GF_PAIR_TABLES x 65536 counters, [predictor][prior << 8 | value] of
                               // neighbouring M32 bytes (CodecStats.addCountsForM32 :150-156), added to with atomics
    int noRoomyRun;            // (set by gf_launch_huffman_decode, round 6) the roomy run is not launched for this batch: the first run
                               // takes the tiles the pre-pass gave to it as well (what it cannot hold goes to the general kernel)
};
constexpr int GF_ANALYSIS_WORDS = 260;
constexpr int GF_PAIR_TABLES = 5;               // one 65536-bin table of byte pairs per predictor code (CodecStats.sB)
// per-tile record of the tree pre-pass: 8 header words (status, leaves, bit position of the first code, longest code,
// single-symbol value or -1, 3 spare), then 256 x (path bits uint64), 256 x code length, 256 x symbol
constexpr int GF_TREE_REC_WORDS = 8 + 512 + 64 + 64;
// fastBytes / roomyBytes (round 5): GfDecodeArgs::ldsM32Bytes / ldsM32Roomy of the decode launch that follows -- the pre-pass marks
// the tiles whose M32 stream or packing outgrows the first but fits the second (GF_TREE_ROOMY in word 3 of the tile's record) and
// lists them (roomyList; count in clearFlags[2]), so that the fast kernel's two runs know their tiles BEFORE either starts and
// can run side by side (GfSideStream)
hipError_t gf_launch_huffman_parse_trees(const uint8_t *blob, size_t blobBytes, const uint64_t *offsets, size_t slotStride,
                                         const uint32_t *lengths, uint32_t *trees, size_t nTiles, hipStream_t stream,
                                         uint32_t *clearFlags = nullptr,      // clearFlags: GfDecodeArgs::retryFlag, words 0 and 1 zeroed by the pre-pass
                                         uint32_t fastBytes = 0, uint32_t roomyBytes = 0, uint32_t *roomyList = nullptr);
constexpr uint32_t GF_TREE_ROOMY = 0x400u;          // word 3 of a tree record (beside GF_TREE_HAS_*): the tile belongs to the roomy run
// A second stream of the context with the two events that fork it off the caller's stream and join it again: the fast decode
// kernel's roomy run (some per cent of the tiles of rough terrain, none of smooth terrain) runs there, beside the first run
// instead of behind it.  Event record / wait only: safe inside a stream capture (the side stream joins the capture and leaves it).
struct GfSideStream {
    hipStream_t stream;
    hipEvent_t fork, join;
};

// What tells the two optimal-predictor codecs apart in a container of CodecM32 bytes (lsop/LsHeader.java:137-189): the number of
// coefficients the header must state and the lengths of the two residual streams.  strictTypes: a container type other than 0 or 1
// is GF_K_ERR_FORMAT (LSOP08); without it type 2 is left to the canonical unpacker and any other type reads as Deflate (LSOP12).
struct GfLsopForm {
    uint32_t nCoef, nInit, nInt;
    int strictTypes;
};
inline GfLsopForm gf_lsop_form(const LsopFamily &F, int nRows, int nCols, int strictTypes)       // (the numbers: gvrs_lsop_container.h)
{
    return GfLsopForm{F.nCoef, (uint32_t)F.nInit(nRows, nCols), (uint32_t)F.nInt(nRows, nCols), strictTypes};
}
inline GfLsopForm gf_lsop12_form(int nRows, int nCols) { return gf_lsop_form(GF_LSOP12, nRows, nCols, 0); }
inline GfLsopForm gf_lsop08_form(int nRows, int nCols) { return gf_lsop_form(GF_LSOP08, nRows, nCols, 1); }

// LSOP containers whose entropy stage is CodecM32 bytes: type 0 (legacy Huffman of the two M32 streams) and, with
// rawM32 = 1, type 1 after the host inflated it (gvrs_decode.hip: k_lsop_unpack_m32)
struct GfLsopM32Args {
    const uint8_t *blob;       // 4-byte aligned
    size_t blobBytes;
    const uint64_t *offsets;   // may be null -> t * slotStride
    size_t slotStride;
    const uint32_t *lengths;
    int32_t *residuals;        // nTiles * resStride ints: initialisers, then interior
    size_t resStride;
    uint32_t *coefs;           // nTiles * 16 words: seed, form.nCoef float bit patterns
    int32_t *status;           // in: only tiles marked GF_K_ERR_UNSUPPORTED are touched; out: their decode status
    uint8_t *workspace;        // gridDim.x * workspaceStride bytes (M32 spill)
    size_t workspaceStride;
    size_t nTiles;
    int nRows, nCols;
    uint32_t ldsM32Bytes;
    int rawM32;                // 1: type-1 containers hold the inflated M32 bytes of both streams behind the header
                               // 2: the inflated M32 bytes of tile t are at rawSide + t * rawSideStride (device inflate)
    const uint8_t *rawSide;
    size_t rawSideStride;
    const int32_t *sideStatus;     // mode 2, per tile (k_lsop_streams): 0 = inflated, < 0 = the first stream's failure
    const uint32_t *produced2;     // mode 2: bytes the second stream gave
    const int32_t *inflStatus2;    // mode 2: the second stream's status
    GfLsopForm form;
};

hipError_t gf_launch_lsop_unpack_m32(const GfLsopM32Args &a, hipStream_t stream, unsigned grid);

// The kernels a batch launched, as bits set in host code at the launch sites (the launchers' `launched` argument, may be null):
// what gf_internal_route_report hands to tests.  Decode: k_huffman_decode<MODE> of the 256-, 512- and 1024-thread builds is bit
// 3 * MODE + build (MODE = DEC_GENERAL 0, DEC_ANALYZE 1, DEC_FAST 2, DEC_FAST_ROOMY 3, DEC_FAST_CANON 4; build 0, 1, 2).
constexpr int GF_RT_DEC_MODE_BITS = 3;
constexpr uint32_t GF_RT_CANON_DEC_T256 = 1u << 15;      // k_canon_decode<false>, 256 threads
constexpr uint32_t GF_RT_CANON_DEC_T512 = 1u << 16;      // ... 512 threads
constexpr uint32_t GF_RT_CANON_ANALYZE = 1u << 17;       // k_canon_decode<true> + k_canon_stats
constexpr uint32_t GF_RT_TREES_1 = 1u << 18;             // k_huffman_parse_trees<1>
constexpr uint32_t GF_RT_TREES_64 = 1u << 19;            // k_huffman_parse_trees<64>
constexpr uint32_t GF_RT_LENGTHS_1 = 1u << 20;           // k_canon_parse_lengths<1>
constexpr uint32_t GF_RT_LENGTHS_64 = 1u << 21;          // k_canon_parse_lengths<64>
__host__ __device__ constexpr uint32_t gf_rt_dec_bit(int mode, int threads)
{
    return 1u << (GF_RT_DEC_MODE_BITS * mode + (threads == 1024 ? 2 : threads == 512 ? 1 : 0));
}
// encode
constexpr uint32_t GF_RT_ENC_SPLIT = 1u << 0;            // k_huffman_encode<true, 1> + k_huffman_trees (the batch form)
constexpr uint32_t GF_RT_ENC_FAST = 1u << 1;             // k_huffman_encode<true> alone
constexpr uint32_t GF_RT_ENC_GENERAL = 1u << 2;          // k_huffman_encode<false> (tiles of 2^23 / 6 cells and more)
constexpr uint32_t GF_RT_ENC_PACK = 1u << 3;             // k_huffman_pack
constexpr uint32_t GF_RT_ENC_PACK_RARE = 1u << 4;        // k_huffman_pack_rare
constexpr uint32_t GF_RT_ENC_LEAN_T1024 = 1u << 5;       // the kernels above from the 1024-thread one-tile build
constexpr uint32_t GF_RT_CANON_ENC_1 = 1u << 6;          // k_canon_encode<1> + k_canon_trees
constexpr uint32_t GF_RT_CANON_ENC_0 = 1u << 7;          // k_canon_encode<0>
constexpr uint32_t GF_RT_CANON_PACK = 1u << 8;           // k_canon_pack
constexpr uint32_t GF_RT_ENC_PLANE = 1u << 9;            // the phase-A kernel wrote the byte plane (GfEncodeArgs::plane)
// The fast decode kernel's roomy run (GfDecodeArgs::ldsM32Roomy): which form gf_launch_huffman_decode* gives it
enum { GF_ROOMY_NONE = 0,      // no roomy budget (ldsM32Roomy == 0): one run of the fast kernel, or none
       GF_ROOMY_BESIDE = 1,    // the roomy run on the caller's stream, the first run on the context's side stream
       GF_ROOMY_BEHIND = 2,    // both runs on the caller's stream, the roomy run first
       GF_ROOMY_SKIPPED = 3 }; // no roomy launch (GfDecodeArgs::noRoomyRun): the first run tries the listed tiles as well

hipError_t gf_launch_huffman_encode(const GfEncodeArgs &a, hipStream_t stream, uint32_t *launched = nullptr);
hipError_t gf_launch_huffman_encode_lean_t1024(const GfEncodeArgs &a, hipStream_t stream, uint32_t *launched = nullptr);   // 1024-thread workgroups, GfEncodeArgs::lean only
// roomyForm: GF_ROOMY_* (gf_internal_route_plan); GF_ROOMY_BESIDE needs side
hipError_t gf_launch_huffman_decode(const GfDecodeArgs &a, hipStream_t stream, unsigned grid, const GfSideStream *side, int roomyForm,
                                    uint32_t *launched = nullptr);
hipError_t gf_launch_huffman_decode_t512(const GfDecodeArgs &a, hipStream_t stream, unsigned grid, const GfSideStream *side, int roomyForm,
                                         uint32_t *launched = nullptr);   // 512-thread workgroups
hipError_t gf_launch_huffman_decode_t1024(const GfDecodeArgs &a, hipStream_t stream, unsigned grid, const GfSideStream *side, int roomyForm,
                                          uint32_t *launched = nullptr);  // 1024-thread workgroups
// CodecCanonHuffman packings without escapes through the fast body (DEC_FAST_CANON in gvrs_decode.hip); the tiles it leaves carry
// GF_K_RETRY and a.retryFlag[0] != 0: k_canon_decode (launched with the same retryFlag) takes those
hipError_t gf_launch_huffman_decode_canon(const GfDecodeArgs &a, hipStream_t stream, uint32_t *launched = nullptr);
hipError_t gf_launch_huffman_decode_canon_t512(const GfDecodeArgs &a, hipStream_t stream, uint32_t *launched = nullptr);
hipError_t gf_launch_huffman_decode_canon_t1024(const GfDecodeArgs &a, hipStream_t stream, uint32_t *launched = nullptr);
size_t gf_huffman_decode_lds_per_wg(const GfDecodeArgs &a);           // LDS bytes per workgroup, 256-thread build
size_t gf_huffman_decode_lds_per_wg_t512(const GfDecodeArgs &a);      // ... 512-thread build
size_t gf_huffman_decode_lds_per_wg_t1024(const GfDecodeArgs &a);     // ... 1024-thread build
unsigned gf_huffman_decode_grid(size_t nTiles);
uint32_t gf_huffman_decode_lds_m32(int nRows, int nCols);
uint32_t gf_huffman_decode_lds_text(int nRows, int nCols);

// per-tile record of the canonical decoder's code-length pre-pass: 8 header words (status, bit position of the text
// relative to the packing, 6 spare), then the 261 code lengths (CanonHuffTreeDecoder.decodeTree) padded to 272 bytes
constexpr int GF_CANON_REC_WORDS = 8 + 68;
hipError_t gf_launch_canon_parse_lengths(const uint8_t *blob, size_t blobBytes, const uint64_t *offsets, size_t slotStride,
                                         const uint32_t *lengths, uint32_t *recs, size_t nTiles, int lsopContainer,
                                         hipStream_t stream, uint32_t *clearFlags = nullptr);   // clearFlags: GfDecodeArgs::retryFlag, zeroed

// CodecCanonHuffman (gvrs_canon_encode.hip / gvrs_canon_decode.hip); same argument blocks as the legacy codec
hipError_t gf_launch_canon_encode(const GfEncodeArgs &a, hipStream_t stream, uint32_t *launched = nullptr);
size_t gf_canon_stat_words();          // words per tile of GfEncodeArgs::encStats for the canonical encoder
size_t gf_canon_pack_rec_words();      // words per tile of GfEncodeArgs::packRecs for the canonical encoder
hipError_t gf_launch_canon_decode(const GfDecodeArgs &a, hipStream_t stream, unsigned grid);
uint32_t gf_canon_decode_lds_text(int nRows, int nCols);
// the 512-thread build of the canonical decoder (gvrs_canon_decode.hip compiled with -DGF_CD_THREADS=512 -DGF_CD_VARIANT)
hipError_t gf_launch_canon_decode_t512(const GfDecodeArgs &a, hipStream_t stream, unsigned grid);
uint32_t gf_canon_decode_lds_text_t512(int nRows, int nCols);
uint32_t gf_canon_decode_lds_stage_t512(int nRows, int nCols);
size_t gf_canon_decode_lds_per_wg(const GfDecodeArgs &a);
size_t gf_canon_decode_lds_per_wg_t512(const GfDecodeArgs &a);
// CodecCanonHuffman.analyze (gvrs_aux.hip): k_canon_decode<true> writes each tile's text -- nRows * nCols values in
// stream order, zero behind the end of the text -- to a.values at a stride of gf_canon_stats_stride(cells) values, k_canon_stats
// counts it into GF_CANON_STAT_WORDS words per tile at a.analysis (see there); the 256-thread build's LDS sizes, a.trees set
constexpr int GF_CANON_STAT_WORDS = 16;
__host__ __device__ inline uint32_t gf_canon_stats_stride(uint32_t nCells) { return (nCells + 3u) & ~3u; }
hipError_t gf_launch_canon_analyze(const GfDecodeArgs &a, hipStream_t stream);
uint32_t gf_lsop_unpack_lds_text(int nRows, int nCols);      // the same for k_lsop_unpack2 (trimmed where that gains a workgroup per CU)
uint32_t gf_canon_decode_lds_stage(int nRows, int nCols);

// status (optional): tiles whose status is not GF_K_OK take no room in the blob
hipError_t gf_launch_compact(size_t nTiles, const uint8_t *slots, size_t slotStride,
                             const uint32_t *lengths, uint64_t *offsets, uint8_t *blob,
                             size_t blobCap, hipStream_t stream, const int32_t *status = nullptr);
hipError_t gf_launch_synth_dem(uint64_t seed, int nRows, int nCols, int64_t tilesPerRow,
                               int64_t tile0, size_t nTiles, int32_t *values, hipStream_t stream, int maskPerMille = 0, int style = 0);

// CodecFloat byte planes (gvrs_float.hip); plane buffer of a tile = ceil(n/8) + 4n bytes at planeStride
hipError_t gf_launch_float_planes_encode(const uint32_t *raw, uint8_t *planes, size_t planeStride, size_t nTiles, int nRows,
                                         int nCols, hipStream_t stream);
hipError_t gf_launch_float_planes_decode(const uint8_t *planes, uint32_t *raw, size_t planeStride, size_t nTiles, int nRows,
                                         int nCols, hipStream_t stream);

// LSOP12 (gvrs_lsop.hip, gvrs_lsop_decode.hip).  residuals: per tile resStride ints [initialisers | interior];
// coefs: per tile 16 words (seed, 12 float bit patterns, 3 spare)
hipError_t gf_launch_lsop_predict(const int32_t *values, int32_t *residuals, size_t resStride, uint32_t *coefs,
                                  int32_t *status, size_t nTiles, int nRows, int nCols, hipStream_t stream);
hipError_t gf_launch_canon_pack2(const int32_t *residuals, size_t resStride, const uint32_t *coefs, const int32_t *inStatus,
                                 uint8_t *out, size_t slotStride, uint32_t *lengths, int32_t *status, size_t nTiles,
                                 uint32_t n0, uint32_t n1, int codecIndex, hipStream_t stream, int valueChecksum = 0,
                                 const uint32_t *hist16 = nullptr);
// the encoder's first kernel with the tile held in LDS as halfwords (round 5): residuals as int16 in the same per-tile regions of
// `residuals`, histogram records (gf_lsop_hist_rec_words() words per tile) for gf_launch_canon_pack2's hist16; status receives
// internal codes that only gf_launch_canon_pack2 understands
bool gf_lsop_predict16_eligible(int nRows, int nCols);
size_t gf_lsop_hist_rec_words();
hipError_t gf_launch_lsop_predict16(const int32_t *values, int32_t *residuals, size_t resStride, uint32_t *coefs, int32_t *status,
                                    uint32_t *hist, size_t nTiles, int nRows, int nCols, hipStream_t stream);
// LsHeader.computeChecksum for a batch: word 13 of every tile's coefficient record (16 words) receives the CRC-32C of its values
hipError_t gf_launch_lsop_value_crc(const int32_t *values, size_t nCells, size_t nTiles, const int32_t *inStatus, uint32_t *coefs,
                                    hipStream_t stream);
hipError_t gf_launch_lsop_reconstruct(const int32_t *residuals, size_t resStride, const uint32_t *coefs, const int32_t *inStatus,
                                      int32_t *values, int32_t *status, size_t nTiles, int nRows, int nCols,
                                      hipStream_t stream, bool planes = false);    // planes: word GF_LSOP_FMT_WORD of a tile's
                                                                                   // coefficient record says where its interior residuals are
// LSOP08 (gvrs_lsop8.hip).  residuals: per tile resStride ints [2 nR + 2 nC - 5 initialisers | (nR - 2)(nC - 2) interior]; coefs: per
// tile 16 words (seed, 8 float bit patterns, 7 words of 0).  The kernels walk the batch with at most GF_LSOP8_GRID_CAP workgroups;
// k_lsop8_reconstruct keeps two rows of the tile in LDS, which bounds nCols.
constexpr unsigned GF_LSOP8_GRID_CAP = 32768;
constexpr int GF_LSOP8_MAX_COLS = 16384;
hipError_t gf_launch_lsop8_predict(const int32_t *values, int32_t *residuals, size_t resStride, uint32_t *coefs, int32_t *status,
                                   size_t nTiles, int nRows, int nCols, hipStream_t stream);
// header + two legacy Huffman segments of the M32 bytes (container type 0); inStatus: k_lsop8_predict's
hipError_t gf_launch_lsop8_pack(const int32_t *residuals, size_t resStride, const uint32_t *coefs, const int32_t *inStatus, uint8_t *out,
                                size_t slotStride, uint32_t *lengths, int32_t *status, size_t nTiles, int nRows, int nCols, int codecIndex,
                                hipStream_t stream);
hipError_t gf_launch_lsop8_reconstruct(const int32_t *residuals, size_t resStride, const uint32_t *coefs, const int32_t *inStatus,
                                       int32_t *values, int32_t *status, size_t nTiles, int nRows, int nCols, hipStream_t stream);

// The interior residuals of a decoded tile as a BYTE PLANE in pipeline order (round 6).  k_lsop_reconstruct_plane walks a tile as
// k_lsop_reconstruct_pipe does, with HALF a wave: lane l (0..31) takes rows 2 + l, 2 + 32 + l, ..., three steps behind lane l - 1, a
// new row every P steps (two tiles share a wave) -- and at step s = 16 b + k a lane wants the residual of ITS cell of that step.
// k_lsop_unpack2 therefore leaves the residuals, which it has in LDS as bytes anyway, in exactly that order: byte (b * 32 + l) * 16 + k
// of the plane belongs to lane l at step 16 b + k (steps at which a lane has no interior cell are holes that nobody writes or looks
// at), so that a lane's sixteen residuals of a round are ONE 16-byte load, a tile's 512 bytes in a row -- where the int32 array
// cost four bytes per residual in 64-byte row pieces on both sides (profiles/hbm_traffic.json of round 5: 1.28 GB written, 2.52 GB
// read for 0.93 GB of values).  The plane lies in the tile's residual slot behind the initialisers (which stay int32); a tile with a
// residual outside -127..127 keeps the int32 array and the old kernels (word GF_LSOP_FMT_WORD of its coefficient record: 0 = int32
// array, 1 = plane).
constexpr uint32_t GF_LSOP_FMT_WORD = 14;
constexpr uint32_t GF_LSOP_PLANE_LANES = 32;       // lanes per tile
constexpr uint32_t GF_LSOP_PIPE_MIN_P = 112;       // lane 31 starts 93 steps into a period; lane 0 reads 2 + 16 columns ahead of it
constexpr uint32_t GF_LSOP_PLANE_FRONT = 96;       // lanes 30 / 31 "write" their columns -93.. before they start: words nobody reads
struct GfLsopPlaneGeom {
    uint32_t P;            // steps between two rows of a lane (a multiple of 16)
    uint32_t nPh;          // rows per lane
    uint32_t sEnd;         // the last step that produces a value
    uint32_t nBlocks;      // 16-step blocks: the plane is nBlocks x 32 lanes x 16 bytes
    uint32_t offWords;     // where the plane starts in the tile's residual slot (int32 words; a multiple of 4)
    uint32_t rowsWords;    // k_lsop_reconstruct_plane's LDS per tile: lane 0's two rows above (interleaved, GF_LSOP_PLANE_FRONT columns in front) ...
    uint32_t ldsBytes;     // ... for the two tiles of a wave, + the wave's value stage (33 words per lane) and the rows' store descriptors
    bool ok;               // the shape takes the plane path at all
};
__host__ __device__ inline GfLsopPlaneGeom gf_lsop_plane_geom(uint32_t nR, uint32_t nC)
{
    GfLsopPlaneGeom g{};
    if (nR < 6u || nC < 32u || nC > 4096u || nR > 1024u) return g;      // (narrow tiles: a row's two ends would share a round; tall ones:
                                                                          // k_lsop_unpack2 keeps the rows' 4 (nR - 2) initialisers in the
                                                                          // 4 KB of its token table)
    const uint32_t nInit = 4u * nR + 2u * nC - 9u, nInt = (nR - 2u) * (nC - 4u), L = GF_LSOP_PLANE_LANES;
    g.P = ((nC > GF_LSOP_PIPE_MIN_P ? nC : GF_LSOP_PIPE_MIN_P) + 15u) & ~15u;
    g.nPh = (nR - 2u + L - 1u) / L;
    const uint32_t nLast = nR - 2u - L * (g.nPh - 1u);
    g.sEnd = (g.nPh - 1u) * g.P + 3u * (nLast - 1u) + nC - 1u;
    g.nBlocks = g.sEnd / 16u + 1u;
    g.offWords = (nInit + 3u) & ~3u;
    g.rowsWords = 2u * (GF_LSOP_PLANE_FRONT + g.P + 32u);
    g.ldsBytes = (2u * g.rowsWords + 64u * 33u + 128u) * 4u;
    g.ok = (uint64_t)g.offWords * 4u + (uint64_t)g.nBlocks * (L * 16u) <= ((uint64_t)nInit + nInt) * 4u && g.ldsBytes <= 64u * 1024u;
    return g;
}
hipError_t gf_launch_lsop_unpack2(const uint8_t *blob, size_t blobBytes, const uint64_t *offsets, size_t slotStride,
                                  const uint32_t *lengths, int32_t *residuals, size_t resStride, uint32_t *coefs,
                                  int32_t *status, size_t nTiles, int nRows, int nCols, uint32_t ldsTextBytes, unsigned grid,
                                  hipStream_t stream, const uint32_t *pre = nullptr,    // pre: records of the first stream's lengths
                                  uint32_t *debug = nullptr,                            // debug: cycle stamps (diagnostic flavour)
                                  uint32_t *pre2 = nullptr,     // room for k_lsop_head's records of the second stream (as many as pre): the
                                                                // serial parts of a tile -- its first stream, the second one's code lengths --
                                                                // then run a lane per tile in front of k_lsop_unpack2
                                  bool planes = false);         // interior residuals as byte planes where a tile allows (see above)

// zlib streams inflated on the GPU, one wave per stream (gvrs_inflate.hip)
struct GfInflateStream {
    uint64_t inOffset;         // the stream (2-byte zlib header first) starts at inBase + inOffset
    uint64_t outOffset;        // its output goes to outBase + outOffset
    uint32_t inLen;            // bytes of input that belong to the stream
    uint32_t outCap;           // room for output (Inflater.inflate(byte[]) semantics: produce at most this much)
};
struct GfInflateArgs {
    const uint8_t *inBase;
    uint8_t *outBase;
    const GfInflateStream *streams;
    uint32_t *produced;        // per stream: bytes written
    int32_t *status;           // per stream: GF_K_OK or GF_K_ERR_FORMAT (what makes Inflater throw DataFormatException)
    size_t nStreams;
    uint32_t window;           // LDS window per wave: gf_inflate_window(largest outCap)
    uint32_t *consumed;        // may be null; per stream: bytes of input used (Inflater.getTotalIn()): where a following stream starts
    const uint32_t *gate;      // may be null; a device word: zero = no stream of this launch has any input, every wave leaves at once
};
uint32_t gf_inflate_window(uint32_t maxOut);
hipError_t gf_launch_inflate(const GfInflateArgs &a, hipStream_t stream);
// container walkers, one thread per tile: stream descriptors of CodecDeflate / CodecFloat packings, status merging
hipError_t gf_launch_deflate_streams(const uint8_t *blob, size_t blobBytes, const uint64_t *offsets, size_t slotStride,
                                     const uint32_t *lengths, size_t tile0, size_t nTiles, uint32_t cells, uint8_t *raw, size_t rawStride,
                                     GfInflateStream *desc, int32_t *pre, hipStream_t stream);
hipError_t gf_launch_deflate_lengths(size_t nTiles, const GfInflateStream *desc, const uint32_t *produced, const int32_t *inflStatus,
                                     int32_t *pre, uint32_t *rawLengths, uint8_t *rawBase, hipStream_t stream);
hipError_t gf_launch_merge_status(size_t nTiles, const int32_t *pre, const int32_t *decoded, int32_t *status, hipStream_t stream);
hipError_t gf_launch_float_streams(const uint8_t *blob, size_t blobBytes, const uint64_t *offsets, const uint32_t *lengths, size_t tile0,
                                   size_t nTiles, uint32_t cells, size_t planeStride, GfInflateStream *desc, int32_t *pre, hipStream_t stream);
hipError_t gf_launch_lsop_streams(const uint8_t *blob, size_t blobBytes, const uint64_t *offsets, size_t slotStride, const uint32_t *lengths,
                                  size_t nTiles, GfLsopForm form, size_t rawStride, int pass, const uint32_t *produced,
                                  const int32_t *inflStatus, const uint32_t *consumed, GfInflateStream *desc, int32_t *side, uint32_t *gate,
                                  hipStream_t stream);
hipError_t gf_launch_float_short_planes(size_t nTiles, const int32_t *pre, const int32_t *inflStatus, const uint32_t *produced,
                                        uint8_t *planes, size_t planeStride, int nRows, int nCols, hipStream_t stream);
hipError_t gf_launch_float_status(size_t nTiles, const int32_t *pre, const int32_t *inflStatus, int32_t *status, hipStream_t stream);

// predictor -> M32 stage alone (gvrs_encode.hip): per tile up to three candidate M32 streams (CodecDeflate.java:157-199)
struct GfM32Args {
    const int32_t *values;
    uint8_t *out;              // per tile 3 sub-slots of subStride bytes (candidates in the order D, L, T; nulls: slot 0)
    size_t subStride;          // multiple of 16
    uint32_t *lengths;         // 3 per tile: M32 bytes of the candidate (0 = not a candidate)
    uint8_t *models;           // 3 per tile: predictor code of the candidate or 0
    uint32_t *seeds;           // 1 per tile
    int32_t *status;           // GF_K_OK / DECLINED / OVERFLOW (a candidate did not fit; its length is still exact) / ERR_BOUNDS
    size_t nTiles;
    int nRows, nCols;
};
hipError_t gf_launch_m32_streams(const GfM32Args &a, hipStream_t stream);

// Tile records and mixed-codec packings in device memory (gvrs_records.hip; driven by gvrs_api_records_dev.hip): one pipeline of
// k_record_parse_elems, k_record_crc32c_elems, k_codec_partition, the codecs' decoders and k_elem_scatter.  A tile record holds one
// or more elements; every per-element array is ELEMENT-MAJOR: instance i = e * nTiles + t is element e of record t, so that
// k_codec_partition sorts the instances of all elements in one run and a codec's decoder is launched once for all of them.
// An instance's class after the framing walk: the index of the codec its packing names, or one of
constexpr int32_t GF_REC_FAILED = -1;        // no element to decode or copy: the instance's status says why
constexpr int32_t GF_REC_STANDARD = 256;     // the standard form: the element bytes are the cells themselves
constexpr int GF_K_MAX_ELEMS = 16;               // (= GF_MAX_ELEMS of the C ABI)
constexpr int GF_K_ELEM_INT = 0, GF_K_ELEM_SHORT = 1, GF_K_ELEM_FLOAT = 2, GF_K_ELEM_ICF = 3;    // (= GF_ELEM_*)
struct GfElemDesc {            // an element of the tile, in device memory for k_elem_scatter (32 bytes)
    void *values;              // nTiles * cells cells: int32 (INT), int16 (SHORT), float32 (FLOAT, ICF)
    int32_t type;              // GF_K_ELEM_*
    int32_t fillI;             // ICF: the stored code of "no data" ...
    float scale, offset;       // ... value = code / scale + offset
    float fillF;               // ... and what a cell equal to fillI is delivered as
    uint32_t pad;
};
struct GfRecordParseElemsArgs {
    const uint8_t *blob;       // 4-byte aligned
    size_t blobBytes;
    const uint64_t *offsets;   // records: nTiles + 1 entries, record t = [offsets[t], offsets[t + 1]); packings: nTiles entries
    const uint64_t *ends;      // records only, may be null; else nTiles entries and record t = [offsets[t], ends[t]): records that lie
                               // anywhere in the blob (a file image), offsets[nTiles] is not read
    const uint32_t *lengths;   // null: tile records with their framing; else packing t = lengths[t] bytes at offsets[t]: no head, no
                               // standard form, no tile index, one INT element
    size_t nTiles;
    int nElems;                // 1 .. GF_K_MAX_ELEMS
    uint32_t elemTypes;        // two bits per element: its GF_K_ELEM_* (no indexed kernel argument)
    uint32_t cells;
    int nCodecs;
    uint64_t intSet0, intSet1, intSet2, intSet3;       // bit k: entry k of the codec list has an integer decoder
    uint64_t floatSet0, floatSet1, floatSet2, floatSet3;   // bit k: entry k is GF_CODEC_NONE, the slot of CodecFloat
    int32_t *tileIndices;      // may be null
    uint64_t *starts;          // per instance: where the element bytes start in the blob
    uint32_t *lens;            // ... how many they are
    int32_t *cls;              // ... its class (GF_REC_FAILED, GF_REC_STANDARD or the index of its codec)
    int32_t *status;           // ... GF_K_OK or the framing's verdict
    uint32_t *sizes;           // per RECORD: its size field when the record is one whose checksum the host call verifies, else 0
                               // (always 0 in packing mode)
};
hipError_t gf_launch_record_parse_elems(const GfRecordParseElemsArgs &a, hipStream_t stream);
// the CRC-32C of every record with sizes[t] != 0; a mismatch: status GF_K_ERR_FORMAT, class GF_REC_FAILED for all nElems instances
hipError_t gf_launch_record_crc32c_elems(const uint8_t *blob, const uint64_t *offsets, const uint32_t *sizes, int32_t *cls, int32_t *status,
                                         size_t nTiles, int nElems, hipStream_t stream);
// stable partition by class: segments 0 .. nCodecs - 1 (the codecs' packings) and nCodecs (standard form) one behind the other
struct GfPartitionArgs {
    const int32_t *cls;
    const uint64_t *starts;
    const uint32_t *lens;
    size_t nTiles;             // instances; < 2^32
    int nCodecs;               // <= 255
    uint64_t *subOffsets;      // nTiles entries each
    uint32_t *subLengths;
    uint32_t *subDst;
    uint32_t *counts;          // nCodecs + 1 entries
};
hipError_t gf_launch_codec_partition(const GfPartitionArgs &a, hipStream_t stream);
struct GfElemScatterArgs {
    const uint8_t *blob;
    const int32_t *tmp;        // decoded tiles (int32 cells or float bit patterns), entry j of the partition at tmp + j * cells
    const int32_t *subStatus;  // their decoders' statuses
    const uint64_t *subOffsets;
    const uint32_t *subDst;    // the entry's instance number
    size_t nPacked;            // entries with a decoded tile; [nPacked, nTotal): elements in standard form
    size_t nTotal;
    size_t nTiles;
    uint32_t cells;
    const GfElemDesc *elems;   // device memory, nElems entries
    int32_t *status;           // per instance
};
hipError_t gf_launch_elem_scatter(const GfElemScatterArgs &a, hipStream_t stream);

// Grid blocks (gvrs_blocks.hip; driven by gvrs_api_blocks.hip): a rectangle of the grid gathered from decoded tiles (k_block_slots,
// k_block_gather: the loops of gvrs/GvrsElement.java:348-402) and a raster cut into tiles (k_grid_cut).  The grid is nRowsOfTiles x
// nColsOfTiles tiles of nRowsTile x nColsTile cells, tile index = tileRow * nColsOfTiles + tileCol (TileAccessIndices.java:86-88);
// every byte address is 64 bits wide.
struct GfBlockGeom {
    int32_t nRowsTile, nColsTile;
    int32_t nColsOfTiles, nTilesGrid;                // nTilesGrid = nRowsOfTiles * nColsOfTiles <= 0x7fffffff
    int32_t row0, col0, nRows, nCols;                // the rectangle, in grid coordinates
    int32_t tileRow0, tileCol0, nTileRows, nTileCols;   // the rectangle of tiles it touches
};
struct GfBlockElem {           // an element of the block, in device memory for k_block_gather (32 bytes)
    const void *tiles;         // decoded tiles of the element, record j at tiles + j * cells items
    void *block;               // nRows * nCols items, row-major
    const int32_t *status;     // may be null; per record: the element's status, anything but GF_K_OK reads as fill
    uint32_t fillBits;         // the fill value's bits (SHORT: the low 16)
    uint32_t itemBytes;        // 2 (SHORT) or 4
};
struct GfBlockSlotsArgs {
    const int32_t *tileIndices;   // per record
    size_t nRecords;              // <= 0x7fffffff
    int32_t *slots;               // nTileRows * nTileCols entries, pre-set to -1: the highest record number of each tile
    GfBlockGeom g;
};
hipError_t gf_launch_block_slots(const GfBlockSlotsArgs &a, hipStream_t stream);
struct GfBlockGatherArgs {
    const int32_t *slots;
    const GfBlockElem *elems;     // device memory, nElems entries; null: the one element of `one` (no table to upload: capture-safe)
    GfBlockElem one;
    int nElems;
    GfBlockGeom g;
};
hipError_t gf_launch_block_gather(const GfBlockGatherArgs &a, hipStream_t stream);
struct GfGridCutArgs {
    const void *block;            // the rectangle's cells, row-major
    void *tiles;                  // listed tile j at tiles + j * cells items
    const int32_t *tileIndices;   // per listed tile: its index in the grid
    int32_t *status;              // may be null; GF_K_OK, or GF_K_ERR_BOUNDS for an index outside [0, nTilesGrid): nothing of it is written
    size_t nTiles;
    uint32_t fillBits, itemBytes;
    int keepOutside;              // != 0: cells outside the rectangle are left as they are
    GfBlockGeom g;
};
hipError_t gf_launch_grid_cut(const GfGridCutArgs &a, hipStream_t stream);

// A file image (gvrs_file.hip; driven by gvrs_api_file.hip): the tile directory read in place for the tiles of a block's rectangle of
// tiles (k_file_locate), and the verdicts put into the statuses behind the records' pipeline (k_file_status).  Slot j = the j-th
// tile of the rectangle of tiles, row-major.  A slot's verdict: GF_K_OK for a tile the file does not hold (the directory's entry
// is 0 or the tile lies outside the directory's rectangle), GF_K_ERR_BOUNDS / GF_K_ERR_FORMAT for an entry that is refused -- all
// three with the empty extent [0, 0), which the framing walk refuses without reading anything -- or
constexpr int32_t GF_FILE_LOCATED = 1;       // the record's extent is emitted: the pipeline's own statuses stand
struct GfFileLocateArgs {
    const uint8_t *image;      // 8-byte aligned
    uint64_t imageBytes;
    GfFileDir dir;             // the tile directory (gvrs_file_parse.h)
    int32_t tileRow0, tileCol0, nTileRows, nTileCols;   // the block's rectangle of tiles: nTileRows * nTileCols <= 0x7fffffff slots
    uint64_t *starts, *ends;   // per slot: the record's extent [position - 8, min(imageBytes, position - 8 + size))
    int32_t *verdict;          // per slot
    uint8_t *present;          // may be null; per slot: 1 where the directory's entry is not 0
    const int32_t *tileList;   // may be null; else slot j = the tile tileList[j] of the grid, j < nList, and the rectangle is not read
    uint32_t nList;            // <= 0x7fffffff
};
hipError_t gf_launch_file_locate(const GfFileLocateArgs &a, hipStream_t stream);
// status[e * nSlots + j] = verdict[j] wherever that is not GF_FILE_LOCATED
hipError_t gf_launch_file_status(const int32_t *verdict, int32_t *status, size_t nSlots, int nElems, hipStream_t stream);

// A file image read at POINTS (gvrs_file_points.hip; driven by gvrs_api_file_points.hip; the arithmetic is gvrs_file_points.h).
// k_points_mark sets the bit of every tile a point needs in a bitmap of one bit per tile of the grid (zeroed by the host): cells
// (rowsI / colsI) or the 4 x 4 windows of interpolation points (rowsD / colsD through gf_interp_window of ig); a refused point
// marks nothing.  k_points_rank, ONE workgroup, writes per word the exclusive prefix of the popcounts, the touched tiles in
// ascending order (at most maxTiles of them) and their count.  The touched tiles' records are then located (k_file_locate over
// the list) and decoded by the records' pipeline into a pool, tile of slot s at pool + s * cells items, and k_points_cells /
// k_points_interp sample the pool: a tile's slot is gf_points_slot(bits, prefix, tile).
constexpr uint32_t GF_POINTS_RANK_CHUNK = 1024;    // words of the bitmap a turn of k_points_rank's loop takes (= its lanes)
struct GfPointsMarkArgs {
    GfPointsGrid g;
    GfInterpGeom ig;           // windows: the whole grid as the block; wrap and the fringes
    size_t nPoints;            // <= 0x7fffffff
    const int32_t *rowsI, *colsI;
    const double *rowsD, *colsD;
    uint32_t *bits;
};
hipError_t gf_launch_points_mark(const GfPointsMarkArgs &a, bool windows, hipStream_t stream);
struct GfPointsRankArgs {
    const uint32_t *bits;
    uint32_t nWords;           // <= 2^22
    uint32_t *prefix;          // nWords
    int32_t *list;             // maxTiles entries
    uint32_t maxTiles;
    uint32_t *count;           // one word: the touched tiles, whatever maxTiles is
};
hipError_t gf_launch_points_rank(const GfPointsRankArgs &a, hipStream_t stream);
struct GfPointsElem {          // an element of the file for k_points_cells
    const void *pool;          // decoded tiles, slot s at pool + s * cells items
    void *values;              // per point, in the delivered type
    uint32_t fillBits, itemBytes;
};
struct GfPointsLookup {        // what both sampling kernels take of the touched tiles
    const uint32_t *bits, *prefix;
    const int32_t *verdict;    // per slot: GF_FILE_LOCATED or what k_file_locate found
    const int32_t *slotStatus; // [e * nSlots + s]: the records' pipeline's, with the verdicts put in (k_file_status)
    uint32_t nSlots, cells;
};
struct GfPointsCellsArgs {
    GfPointsGrid g;
    GfPointsLookup look;
    size_t nPoints;
    const int32_t *rows, *cols;
    int32_t *status;           // [e * nPoints + i]
    int nElems;
    GfPointsElem elems[GF_K_MAX_ELEMS];
};
hipError_t gf_launch_points_cells(const GfPointsCellsArgs &a, hipStream_t stream);
struct GfPointsInterpArgs {
    GfPointsGrid g;
    GfInterpGeom ig;           // the whole grid as the block; the element's type and fill
    GfPointsLookup look;       // slotStatus: the element's row of it
    const void *pool;          // the element's
    uint32_t fillBits;
    size_t nPoints;
    const double *rows, *cols, *colSpacing;
    double *z, *zx, *zy, *zxx, *zxy, *zyy, *normal;
    int32_t *status;
};
hipError_t gf_launch_points_interp(const GfPointsInterpArgs &a, hipStream_t stream);

// A file queried at COORDINATES (the rules are gvrs_coords.h).  k_coords_map (gvrs_coords.hip), a lane per point, is
// gf_coords_map over a batch: the direction and the outputs that were passed are wave-uniform branches, every output item is
// written exactly once.  The fused forms are second instantiations of k_points_mark<true> and k_points_interp
// (gvrs_file_points.hip): point t is gf_coords_query of (m.rowsD[t], m.colsD[t]) / (p.rows[t], p.cols[t]), given as kind says,
// mapped in registers; the body behind it is the one the grid-coordinate instantiations run.  p.colSpacing, where not null,
// replaces the rule's spacing; a point the latitude check refuses is GF_K_ERR_ARG with NaN outputs and marks nothing.
struct GfCoordsMapArgs {
    GfCoords c;
    int32_t kind;              // GF_CO_GEO_TO_GRID .. GF_CO_GRID_TO_MODEL
    size_t nPoints;
    const double *a, *b;
    double *outA, *outB;
    int32_t *iRow, *iCol;      // may be null; to-grid kinds only
    double *colSpacing;        // may be null; to-grid kinds only
    int32_t *status;           // may be null; to-grid kinds only
};
hipError_t gf_launch_coords_map(const GfCoordsMapArgs &a, hipStream_t stream);
struct GfPointsMarkCoordsArgs {
    GfPointsMarkArgs m;        // rowsD / colsD: the points' a / b
    GfCoords c;
    int32_t kind;              // GF_CO_GRID, GF_CO_FILE
};
hipError_t gf_launch_points_mark_coords(const GfPointsMarkCoordsArgs &a, hipStream_t stream);
struct GfPointsInterpCoordsArgs {
    GfPointsInterpArgs p;      // rows / cols: the points' a / b; ig.colSpacing: du
    GfCoords c;
    int32_t kind;
    double *colSpacingUsed;    // may be null; per point the spacing it was evaluated with, NaN for a refused point
};
hipError_t gf_launch_points_interp_coords(const GfPointsInterpCoordsArgs &a, hipStream_t stream);

// A file image WRITTEN at points (gvrs_file_points_write.hip; driven by gvrs_api_file_points.hip; the cell rule is
// gvrs_file_points_store.h).  Behind mark, rank and k_file_locate, k_points_heads judges the head of every located record as an
// update does (gfFsHeadWords: a refused one becomes its slot's verdict and the empty extent); behind the records' pipeline and
// k_file_status, k_points_prepare folds the elements' statuses into one per slot, clears the slot's "stored" flag and fills the
// pool slots of the tiles without a record; k_points_claim lets the highest point index whose value passed own a cell
// (atomicMax into the element's owner plane, pre-zeroed, one word per pool cell); k_points_store lets the owners store, writes
// the points' statuses and sets the tiles' flags; k_points_verdict writes the touched tiles' indices and the pre-status that the
// record writer takes.  Every index into pool, planes and flags is slot * cells + indexInTile with slot < nSlots and indexInTile
// < cells, or slot < nSlots.
struct GfPointsHeadsArgs {
    const uint8_t *image;      // 8-byte aligned
    uint64_t imageBytes;
    uint64_t *starts, *ends;   // per slot, as k_file_locate left them
    int32_t *verdict;
    uint32_t nSlots;
};
hipError_t gf_launch_points_heads(const GfPointsHeadsArgs &a, hipStream_t stream);
struct GfPointsWriteElem {     // an element of the file, in the kernel arguments
    void *pool;                // decoded tiles in the record writer's type (an ICF's: codes), slot s at pool + s * cells items
    const void *values;        // per point: int32 (INT), int16 (SHORT), float32 (FLOAT and the VALUES of an ICF)
    uint32_t *owner;           // one word per pool cell, pre-zeroed: the highest point index + 1 whose value passed
    int32_t type;              // GF_K_ELEM_*
    uint32_t fillBits, fillFBits, minBits, maxBits;   // as GfBlockCutElem's
    float scale, offset;
};
struct GfPointsWriteArgs {
    GfPointsGrid g;
    GfPointsLookup look;       // slotStatus: the records' pipeline's, with the verdicts put in (k_file_status)
    size_t nPoints;
    const int32_t *rows, *cols;
    int32_t *pointStatus;      // [e * nPoints + i]
    const int32_t *list;       // the touched tiles, ascending: slot s is tile list[s]
    int32_t *slotOld;          // per slot: the first element status that is not GF_K_OK (the tile cannot be rewritten), else GF_K_OK
    uint32_t *stored;          // per slot: != 0 once a point stored a value of any element into the tile
    int32_t *tileIndices;      // out, per slot
    int32_t *preStatus;        // out, per slot: what the record writer takes
    int nElems;
    GfPointsWriteElem elems[GF_K_MAX_ELEMS];
};
hipError_t gf_launch_points_prepare(const GfPointsWriteArgs &a, hipStream_t stream);
hipError_t gf_launch_points_claim(const GfPointsWriteArgs &a, hipStream_t stream);
hipError_t gf_launch_points_store(const GfPointsWriteArgs &a, hipStream_t stream);
hipError_t gf_launch_points_verdict(const GfPointsWriteArgs &a, hipStream_t stream);

// A file image WRITTEN (gvrs_file_write.hip; driven by gvrs_api_file_write.hip): behind the record writer, which has laid the records
// of the rectangle's tiles into the image from firstRecordPos on and left their offsets, the kernels find the bounding rectangle of
// the tiles with a record (k_file_dir_rect), write the tile directory (k_file_dir_entries), checksum it in chunks (k_file_dir_crc)
// and finish the image (k_file_finish).  Slot j = the j-th tile of the rectangle of tiles, row-major; record j is
// image[firstRecordPos + offsets[j] .. firstRecordPos + offsets[j + 1]).
struct GfFileWriteState {      // zeroed before k_file_dir_rect; 0 in the first four words = no tile has a record
    uint32_t invRow0, invCol0; // max of ~row, ~col over the tiles with a record
    uint32_t row1p, col1p;     // max of row + 1, col + 1
    uint32_t extended;         // a record's content position exceeds 1 << 35
    uint32_t pad_[3];
};
struct GfFileWriteArgs {
    uint8_t *image;            // 8-byte aligned
    uint64_t imageCap;
    uint64_t firstRecordPos;   // a multiple of 8
    uint64_t contentPos;       // the header record's end: its checksum word lies 4 bytes in front of it
    const uint64_t *offsets;   // nTileRows * nTileCols + 1
    const uint8_t *metaDir;    // the metadata directory's record, whole (8-byte aligned), metaDirBytes (a multiple of 8, may be 0)
    uint32_t metaDirBytes;
    int32_t checksums, forceExtended;
    int32_t tileRow0, tileCol0, nTileRows, nTileCols;   // the block's rectangle of tiles
    GfFileWriteState *state;
    uint32_t *chunkCrc;        // one word per GF_FILE_CRC_CHUNK bytes of the largest directory the rectangle of tiles can give
    uint64_t *imageBytes;      // out: the image's size, or the size it needs
    int32_t *fileStatus;       // out: GF_K_OK or GF_K_ERR_CAPACITY
};
#define GF_K_ERR_CAPACITY (-3)
// A front of up to this many bytes -- the image's bytes [16, firstRecordPos) and behind them the metadata directory's record --
// travels in k_file_finish's ARGUMENTS: nothing is uploaded and the call waits for nothing.  A longer one (large metadata) is
// copied to the image and to metaDir from a page-locked buffer before the kernels.
constexpr uint32_t GF_FILE_FRONT_ARG_BYTES = 3072;
struct GfFileFinishArgs {
    GfFileWriteArgs a;         // (a.metaDir is not read)
    uint32_t front[GF_FILE_FRONT_ARG_BYTES / 4];
};
// the four kernels, in order; front: null, or the (firstRecordPos - 16 + metaDirBytes) bytes that travel as arguments
hipError_t gf_launch_file_write(const GfFileWriteArgs &a, const uint8_t *front, hipStream_t stream);

// A file image UPDATED IN PLACE (gvrs_file_update.hip; driven by gvrs_api_file_update.hip): records in device memory placed into an
// image that holds the old file.  k_update_snapshot copies the old directory's entries aside, k_update_alloc (one wave) runs the
// allocator of gvrs_file_update.h over the records in order and the close sequence's three allocations and writes NOTHING into
// the image; every kernel behind it reads its verdict and writes only when it is GF_K_OK.
struct GfFileUpdateState {     // k_update_alloc's result
    int32_t verdict;           // GF_K_OK, GF_K_ERR_CAPACITY (total = the size needed) or what refused the call (total 0)
    uint32_t extended, row0, col0, nRows, nCols;   // the new directory
    uint32_t nFinal, hasFreeDir;                   // the final list's nodes; the file gets a free-space directory
    uint64_t total, metaDirAt, tileDirAt, tileDirSize, freeDirAt, freeDirSize;   // record positions (not content positions)
};
constexpr uint64_t GF_UPDATE_UNTOUCHED = ~0ull;   // recPos of a record that changes nothing
constexpr uint32_t GF_UPDATE_LDS_NODES = 2048;    // a list of up to this capacity lives in LDS (32 KiB), a larger one in scratch
struct GfFileUpdateArgs {
    uint8_t *image;            // 8-byte aligned; the old image in its first oldBytes bytes
    uint64_t imageCap, oldBytes;
    GfFileDir dir;             // the OLD tile directory (gvrs_file_parse.h)
    int32_t nTilesGrid;
    int32_t checksums, compression, forceExtended;
    int64_t timeModified;
    const uint8_t *blob;       // 8-byte aligned
    const uint64_t *offsets;   // nRecords + 1
    const int32_t *tiles, *status;   // status may be null
    int32_t *tileStatus;       // may be null; else (the block form) a refused old record gives its tile that status and the tile stays
    uint64_t nRecords, blobBytes;
    GfFileUpdateState *state;
    uint64_t *recPos;          // nRecords: the content position a record got, 0 for a tile freed, GF_UPDATE_UNTOUCHED
    uint64_t *listPos, *listSize, *listPrefix;   // listCap (+ 1 for the prefix sums of the final sizes); the opened list on entry
    uint32_t listCap, nOpened;
    uint64_t *grid;            // nTilesGrid: the old entry of every tile of the grid, then patched with recPos
    uint32_t *seen;            // nTilesGrid, zeroed: how many records name a tile
    const uint8_t *metaDir;    // the old metadata directory's record (8-byte aligned), metaDirBytes (a multiple of 8, may be 0)
    uint32_t metaDirBytes;
    uint32_t *chunkCrc;        // one word per GF_FILE_CRC_CHUNK bytes of the largest directory the grid can give
    uint64_t *imageBytes;      // out
    int32_t *fileStatus;       // out
};
hipError_t gf_launch_file_update(const GfFileUpdateArgs &a, hipStream_t stream);

// A block WRITTEN (gvrs_blocks_write.hip; driven by gvrs_api_blocks_write.hip): the rectangle's cells of every element cut into the
// tiles of the rectangle of tiles in the type the record writer takes (k_block_cut_elems: TileElement*.setValue with its range
// checks, RasterTile.hasValidData), and the per-tile verdict the record writer receives as its pre-status (k_block_write_verdict).
constexpr uint32_t GF_BW_FLAG_BOUNDS = 1u, GF_BW_FLAG_VALID = 2u;   // a tile's flags word: a cell out of range; a cell that is not fill
struct GfBlockCutElem {        // an element of the block, in the kernel arguments (56 bytes): nothing is uploaded, so the call only enqueues
    const void *block;         // nRows * nCols items, row-major: int32 (INT), int16 (SHORT), float32 (FLOAT and the VALUES of an ICF)
    void *tiles;               // tile k of the rectangle of tiles at tiles + k * cells items: int32, int16, float bits, int32 codes
    const void *oldTiles;      // may be null; decoded tiles of the old records in the tiles' type, record j at oldTiles + j * cells items
    int32_t type;              // GF_K_ELEM_*
    uint32_t fillBits;         // what a tile holds where nothing was written: fill_i (SHORT: the low 16 bits; ICF: the code), fill_f's bits
    uint32_t fillFBits;        // ICF: fill_f's bits, the VALUE that converts to the code fillBits
    uint32_t minBits, maxBits; // the accepted range: int32 for INT and SHORT, float bits for FLOAT and ICF
    float scale, offset;       // ICF: code = floor((v - offset) * scale + 0.5)
    uint32_t pad_;
};
struct GfBlockCutElemsArgs {
    int nElems;
    const int32_t *slots;         // may be null (no old records); per tile of the rectangle of tiles: the winning old record or -1
    uint32_t *flags;              // per tile of the rectangle of tiles, pre-zeroed: GF_BW_FLAG_* of all elements, by atomicOr
    GfBlockGeom g;
    GfBlockCutElem elems[GF_K_MAX_ELEMS];
};
hipError_t gf_launch_block_cut_elems(const GfBlockCutElemsArgs &a, hipStream_t stream);
struct GfBlockWriteVerdictArgs {
    const uint32_t *flags;
    const int32_t *slots;         // may be null
    const int32_t *oldStatus;     // with slots: the old records' statuses, element-major [e * nOld + record]
    size_t nOld;
    int nElems;
    int32_t *preStatus;           // per tile: 0, or what the tile gets in place of a record (old-record failure, ERR_BOUNDS, DECLINED)
    int32_t *tileIndices;         // per tile: its index on the grid
    GfBlockGeom g;
};
hipError_t gf_launch_block_write_verdict(const GfBlockWriteVerdictArgs &a, hipStream_t stream);

// Tile records written in device memory (gvrs_records_enc.hip; driven by gvrs_api_records_enc.hip): the mirror image of the read
// side above.  Every integer codec of the list has encoded every integer element of every tile into a slot of its own (a
// CANDIDATE: candidate a of an element is the a-th integer codec of the list); k_record_plan picks the winners and lays the
// records out, k_record_scan turns their sizes into offsets, k_record_write assembles the bytes and k_record_crc32c_write
// checksums them.  Per-element arrays are element-major as on the read side (instance i = e * nTiles + t).
struct GfRecEncElem {          // an element of the tile, in the kernel arguments (32 bytes)
    const void *values;        // the caller's cells, nTiles * cells items: the source of the standard form
    const uint8_t *slots;      // candidate a of tile t: slots + (a * nTiles + t) * slotStride; null: the element has no candidates
    uint32_t stdSize;          // bytes of the standard form (TileElement.java:86-93)
    uint32_t srcBytes;         // bytes of a tile's cells in `values`: stdSize, or stdSize - 2 for a SHORT tile with an odd cell count
    uint32_t slotStride;       // multiple of 16, >= stdSize: a packing that overflowed its slot could not have won
    uint32_t cand0;            // the element's candidates are entries cand0 .. cand0 + nAct - 1 of candLen / candStatus
};
struct GfRecordPlanArgs {
    size_t nTiles;
    int nElems;                // 1 .. GF_K_MAX_ELEMS
    int nAct;                  // integer codecs in the list (0: everything is in standard form)
    const uint32_t *candLen;   // per candidate array and tile [c * nTiles + t]: what the codec's encoder left in d_lengths ...
    const int32_t *candStatus; // ... and in d_status
    uint32_t *elemLen;         // per instance: n, the element's bytes in the record
    uint32_t *elemPos;         // ... where its length word lies in the record
    uint8_t *elemSrc;          // ... the winning candidate, or 255: the standard form
    uint32_t *sizes;           // per record: its size, 0 for a record that is not written (an encoder failed)
    int32_t *status;           // per record: GF_K_OK or the first negative encoder status (element order, then list order)
    uint8_t *codecUsed;        // may be null; per instance: the winner's index in the codec list, or 255
    const int32_t *preStatus;  // may be null; per record, non-zero: the record is not written (size 0), its status is this value and
                               // its codecUsed entries are 255, whatever the encoders said (a block write's verdict on the tile)
    uint8_t actIndex[256];     // candidate a is entry actIndex[a] of the codec list
    GfRecEncElem elems[GF_K_MAX_ELEMS];
};
hipError_t gf_launch_record_plan(const GfRecordPlanArgs &a, hipStream_t stream);
// offsets[0 .. nTiles] = exclusive 64-bit scan of sizes
hipError_t gf_launch_record_scan(const uint32_t *sizes, uint64_t *offsets, size_t nTiles, hipStream_t stream);
struct GfRecordWriteArgs {
    size_t nTiles;
    int nElems;
    int checksum;              // != 0: the last word of a record is left to k_record_crc32c_write, else it is written as 0
    const int32_t *tileIndices;
    const uint32_t *elemLen, *elemPos;
    const uint8_t *elemSrc;
    const uint32_t *sizes;
    const uint64_t *offsets;   // nTiles + 1 entries, multiples of 8
    uint8_t *blob;             // 8-byte aligned
    size_t blobCap;            // a record that would end behind it is skipped whole
    GfRecEncElem elems[GF_K_MAX_ELEMS];
};
hipError_t gf_launch_record_write(const GfRecordWriteArgs &a, hipStream_t stream);
// the CRC-32C of the first size - 4 bytes of every written record into its last word
hipError_t gf_launch_record_crc32c_write(uint8_t *blob, size_t blobCap, const uint64_t *offsets, const uint32_t *sizes, size_t nTiles,
                                         hipStream_t stream);
// SHORT cells widened for the codecs: fill -> INT4_NULL_CODE (TileElementShort.java:211-219).  src 4-byte, dst 16-byte aligned
hipError_t gf_launch_elem_widen(const int16_t *src, int32_t *dst, size_t nCells, int fill, hipStream_t stream);

// B-spline interpolation over a grid block in device memory (gvrs_interp.hip; driven by gvrs_api_interp.hip): a lane per point.
// Points form: rows / cols (and colSpacing, may be null: g.colSpacing) per point.  Lattice form (rows == null): point t is
// (i, j) = (t / latCols, t % latCols), row = latRow0 + (double)i * latRowStep, col = latCol0 + (double)j * latColStep, each one
// product and one sum, and colSpacing (may be null) is per lattice ROW.  Every output pointer may be null except z; normal holds 3
// items per point.  Every output item of every point is written exactly once.  gf_launch_interp sends a lattice with one column
// spacing to k_interp_lattice (a workgroup per patch of the output), everything else to k_interp_points.
struct GfInterpArgs {
    GfInterpGeom g;
    const void *block;
    size_t nPoints;
    const double *rows, *cols, *colSpacing;
    double latRow0, latCol0, latRowStep, latColStep;
    uint64_t latRows, latCols;
    double *z, *zx, *zy, *zxx, *zxy, *zyy, *normal;
    int32_t *status;
};
hipError_t gf_launch_interp(const GfInterpArgs &a, hipStream_t stream);

// A grid block rendered to ARGB words (gvrs_render.hip; driven by gvrs_api_render.hip).  The palette is a packed table in device
// memory (gvrs_render_common.h): head travels by value; table is what lies behind it, keys[n] | recs[n] as 10 n doubles, staged
// in LDS by every workgroup (80 bytes a record).  unlimited: the UnlimitedRange forms of the lookup.
struct GfRenderPal {
    GfPalHead head;
    const double *table;
    int32_t unlimited;
};
// cells form: nCells cells of a block (int32 / int16 / float32 as elemType says; GF_RENDER_ELEM_Z: doubles; aligned to the item) -> argb; shade (may be null):
// one double per cell, the WithShade forms.  Every argb item is written exactly once.
struct GfRenderCellsArgs {
    GfRenderPal pal;
    int32_t elemType, fillI;
    const void *cells;
    const double *shade;
    uint32_t *argb;
    size_t nCells;
};
hipError_t gf_launch_render_cells(const GfRenderCellsArgs &a, hipStream_t stream);
// interpolating forms: ip is what gf_launch_interp takes (its output pointers unused; g.target is GF_IP_FIRST with a light,
// GF_IP_VALUE without); argb, shade and status may each be null.  A lattice with one column spacing goes to k_render_lattice,
// everything else to k_render_points.
struct GfRenderArgs {
    GfInterpArgs ip;
    GfRenderPal pal;
    GfRenderLight light;
    int32_t lit;                                    // != 0: light holds the illumination model; else the lookup without shade
    uint32_t *argb;
    double *shade;
    int32_t *status;
};
hipError_t gf_launch_render(const GfRenderArgs &a, hipStream_t stream);

// A grid block in device memory averaged down by an integer factor (gvrs_downsample.hip; driven by gvrs_api_downsample.hip): block
// and out hold int32 / int16 / float32 cells as g.elemType says, out g.outRows x g.outCols of them, each written exactly once.
// path: GF_DS_AUTO takes what gf_downsample_path chooses -- k_downsample_direct up to GF_DS_DIRECT_MAX_FACTOR, k_downsample_staged
// above it (the measurements behind the bound: DESIGN.md section 4) -- GF_DS_DIRECT / GF_DS_STAGED force one; both serve every
// factor and every geometry, bit for bit alike.
enum { GF_DS_AUTO = 0, GF_DS_DIRECT = 1, GF_DS_STAGED = 2 };
constexpr int32_t GF_DS_DIRECT_MAX_FACTOR = 8;
struct GfDownsampleArgs {
    GfDsGeom g;
    const void *block;
    void *out;
};
int gf_downsample_path(const GfDownsampleArgs &a);
hipError_t gf_launch_downsample(const GfDownsampleArgs &a, int path, hipStream_t stream);

// Packed ARGB words split into three element planes and joined from them (gvrs_image.hip; driven by gvrs_api_image.hip; the
// arithmetic: gvrs_image_common.h).  argb: nPixels words, 4-byte aligned; planes[k]: nPixels int32 (elemType 0, 4-byte aligned) or
// int16 (elemType 1, 2-byte aligned).  Split reads argb and writes the planes, join the reverse; every output item is written
// exactly once and nothing outside the nPixels items is touched.  The box average of packed words goes through
// gf_launch_downsample with g.elemType = GF_DS_ARGB.
struct GfImageArgs {
    int32_t model;                 // GF_IMAGE_MODEL_*
    int32_t elemType;              // 0 INT, 1 SHORT
    size_t nPixels;
    const void *argb;              // (join writes it)
    const void *planes[3];         // (split writes them)
};
hipError_t gf_launch_image_split(const GfImageArgs &a, hipStream_t stream);
hipError_t gf_launch_image_join(const GfImageArgs &a, hipStream_t stream);

// A grid block in device memory tabulated (gvrs_tabulate.hip; driven by gvrs_api_tabulate.hip; the arithmetic: gvrs_tabulate_common.h).
// Dense form: counter[0 .. g.nCounter] are ADDED to (the caller zeroes them unless it accumulates), partials is room for
// GF_TAB_MAX_GROUPS entries, and k_tabulate_finish writes *summary whole (accumulate: merged with what it held).
struct GfTabPartial {          // what a workgroup of k_tabulate_dense leaves for k_tabulate_finish (64 bytes)
    uint64_t nSkipped, nSamples, sumSamples, sumI;
    double mn, mx;             // exact for every element type
    int64_t mnAt, mxAt;        // -1: none
};
struct GfTabDenseArgs {
    GfTabDenseGeom g;
    const void *block;         // int32 / int16 / float32 cells as g.elemType says, 4-byte aligned
    int32_t *counter;
    GfTabPartial *partials;
    GfTabSummary *summary;
    int accumulate;
};
hipError_t gf_launch_tabulate_dense(const GfTabDenseArgs &a, hipStream_t stream);
// Symbol form: the n >= 1 cells as 32-bit symbols, sorted (unsigned) and run-length counted.  keysA: n + 1 words, keysB: n words,
// hist / sums / heads: gf_tab_sort_plan(n)'s histWords / sumWords / nRunBlocks words, nSym: one word; symbols / counts: cap
// entries each (null with cap == 0); *summary is written whole.
struct GfTabSortPlan {
    uint32_t share, nWg;       // keys of a sort workgroup, sort workgroups
    size_t histWords, sumWords, nRunBlocks;
};
GfTabSortPlan gf_tab_sort_plan(uint32_t n);
struct GfTabSymbolsArgs {
    int32_t elemType;
    const void *block;
    uint32_t n;
    uint32_t *keysA, *keysB, *hist, *sums, *heads, *nSym;
    uint32_t *symbols;
    int32_t *counts;
    size_t cap;
    GfTabSymbols *summary;
};
hipError_t gf_launch_tab_symbols(const GfTabSymbolsArgs &a, hipStream_t stream);
// Two symbol tables merged (gvrs_tabulate_common.h states the rule).  A table's length is read on the device: min(n_written of its
// summary, its cap), 0 with a null summary (and, with its bit of noSamplesIsEmpty set -- 1: A, 2: B --, with n_samples == 0); caps
// up to 2^31 - 1.  splits: gf_tab_merge_chunks(capA, capB) + 1 words, heads: one fewer, sums: that / GF_TAB_SCAN_BLOCK rounded up,
// nSym: one word;
// symbols / counts: cap entries each (null with cap == 0), disjoint from the inputs; *summary is written whole.
struct GfTabMergeArgs {
    const uint32_t *symA, *symB;
    const int32_t *cntA, *cntB;
    const GfTabSymbols *sumA, *sumB;
    uint32_t capA, capB, noSamplesIsEmpty;
    uint32_t *splits, *heads, *sums, *nSym;
    uint32_t *symbols;
    int32_t *counts;
    size_t cap;
    GfTabSymbols *summary;
};
size_t gf_tab_merge_chunks(uint32_t capA, uint32_t capB);
hipError_t gf_launch_tab_merge(const GfTabMergeArgs &a, hipStream_t stream);
// The symbol form of a SHORT block of n >= 1 cells (2-byte aligned) by 65,536 counters, without widening or sorting.  counter:
// 65,536 words (zeroed here); symbols / counts: cap entries each (null with cap == 0); *summary is written whole.
struct GfTabShortArgs {
    const void *block;
    uint32_t n;
    int32_t *counter;
    uint32_t *symbols;
    int32_t *counts;
    size_t cap;
    GfTabSymbols *summary;
};
hipError_t gf_launch_tab_short(const GfTabShortArgs &a, hipStream_t stream);
