// gvrs_api_route.hip -- the route plan and the device-resident batch entry points of CodecHuffman, CodecCanonHuffman and the raw
// M32 streams (what bench.py measures), compaction and the synthetic terrain.

#include "gvrs_api_internal.h"

// ------------------------------------------------------------------ route plan
// Every host decision that picks a kernel build or form for a batch, in one pure function (no device, no HIP call):
// encodeBatchDev and decodeBatchDev launch what it returns, and compare what their launchers report with its bits.  Exported for
// the tests (gf_internal_route_plan, loaded by name; not part of include/gvrs_hip_codec.h): they sweep tile shapes on a machine
// without a device and check on the GPU that each build ran where the plan says.
struct gf_route_plan {
    int32_t decThreads;     // k_huffman_decode build (256, 512, 1024) of the batch -- the canonical run's where viaFast; 0: none
    int32_t viaFast;        // CodecCanonHuffman: the canonical run of the fast kernel (DEC_FAST_CANON) goes before k_canon_decode
    uint32_t fastM32;       // GfDecodeArgs::ldsM32Bytes of the fast kernel's (first) run
    uint32_t ldsM32Roomy;   // GfDecodeArgs::ldsM32Roomy: the roomy run's M32 capacity, 0 without one
    int32_t canonThreads;   // k_canon_decode build (256, 512); 0: none
    int32_t prepass;        // tiles per wave of the pre-pass (1 or 64, gf_prepass_tiles_per_wave); 0: none
    int32_t roomyForm;      // GF_ROOMY_*
    int32_t leanEncode;     // the one-tile path encodes with the 1024-thread build (6 * cells < 2^23)
    uint32_t decBits;       // GF_RT_* of every kernel a decode call launches
    uint32_t encBits;       // GF_RT_* of every kernel an encode call launches
};

// workgroups of a build a CU holds by LDS: 160 KB handed out in 1,280-byte steps, at most cap
static size_t decWgsPerCu(size_t lds, size_t cap)
{
    const size_t step = 1280, n = (160 * 1024) / ((lds + step - 1) / step * step);
    return n < cap ? n : cap;
}

// kind: KIND_HUFFMAN, KIND_CANON or KIND_RAW_M32 (decode only).  roomySeen: the context's hint word (GfDecodeArgs::roomySeenHost,
// 0 where there is none); side: the context has its second stream.
static gf_status routePlan(int kind, int nRows, int nCols, size_t nTiles, int lean, int analysis, uint32_t roomySeen, int side,
                           gf_route_plan &p)
{
    p = gf_route_plan{};
    if (nRows < 1 || nCols < 1 || (kind != KIND_HUFFMAN && kind != KIND_CANON && kind != KIND_RAW_M32)) return GF_ERR_ARG;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    const bool smallEnc = 6ull * cells < (1ull << 23);
    // ---- encode
    if (kind == KIND_CANON) {
        // (encodeBatchDev always hands the canonical encoder its statistics records: the <1> + k_canon_trees form)
        p.encBits = GF_RT_CANON_ENC_1 | GF_RT_CANON_PACK;
        if (!lean) p.encBits |= GF_RT_ENC_PLANE;
    } else if (kind == KIND_HUFFMAN) {
        p.leanEncode = lean && smallEnc;
        if (p.leanEncode) p.encBits = GF_RT_ENC_LEAN_T1024 | GF_RT_ENC_FAST | GF_RT_ENC_PACK;
        else {
            if (smallEnc) {
#ifdef GF_DIAG
                const bool split = !lean && getenv("GF_DIAG_SPLIT") != nullptr;
#else
                const bool split = !lean;
#endif
                p.encBits = split ? GF_RT_ENC_SPLIT : GF_RT_ENC_FAST;
                if (split) p.encBits |= GF_RT_ENC_PLANE;
            } else p.encBits = GF_RT_ENC_GENERAL;
            p.encBits |= GF_RT_ENC_PACK | (lean ? 0u : GF_RT_ENC_PACK_RARE);
        }
    }
    // ---- decode
    p.fastM32 = gf_huffman_decode_lds_m32(nRows, nCols);
    // the k_huffman_decode build.  Occupancy is set by LDS (M32 stream + start bitmap + tables per workgroup), handed out in
    // 1,280-byte steps, and the kernel gains from every wave a CU can hold (tools/occupancy_sweep.sh).  Three builds of the same
    // source: 256 threads (two Huffman cursors per thread in lockstep, the leaner one per wave), 512 threads (one cursor per thread,
    // 64 VGPRs, up to four workgroups = all 32 wave slots of a CU) and 1024.  The 512-thread build is the faster one where it holds
    // at least 1.5 times the waves: measured 120x150 (16 against 32 waves) 1.37 -> 1.19 ms per 12,960 tiles, 100x120 1.59 -> 1.36,
    // 200x200 (8 / 16) 3.92 -> 2.89; 70x100 (24 / 32) 1.62 against 1.81 and 32x32 2.63 against 3.45: the 256-thread build stays.
    // 1024 threads where that doubles the waves again (squares from 167x167 on, but for 208x208..218x218: two workgroups of 512 at
    // most on a CU; tests/test_route_plan.py holds the map).
    // One tile per call: the workgroup is alone on the chip and every phase is a latency chain -- the widest build (120x150:
    // 89 -> 82 us per call against the 512-thread build, 111 with 256 threads).
    auto huffmanBuild = [&](uint32_t ldsM32, uint32_t ldsText) {
        GfDecodeArgs f{};
        f.ldsM32Bytes = ldsM32;
        f.ldsTextBytes = ldsText;
        const size_t waves256 = 4 * decWgsPerCu(gf_huffman_decode_lds_per_wg(f), 8),
                     waves512 = 8 * decWgsPerCu(gf_huffman_decode_lds_per_wg_t512(f), 4),
                     waves1024 = 16 * decWgsPerCu(gf_huffman_decode_lds_per_wg_t1024(f), 2);
        int threads = 2 * waves512 >= 3 * waves256 ? 512 : 256;
        if (threads == 512 && waves1024 >= 2 * waves512) threads = 1024;
        return threads;
    };
    if (kind == KIND_CANON) {
        p.prepass = (int32_t)gf_prepass_tiles_per_wave(nTiles);
        p.decBits = p.prepass == 1 ? GF_RT_LENGTHS_1 : GF_RT_LENGTHS_64;
        // The canonical run of the fast legacy kernel first (round 5): a packing whose code has no escape, null or spare symbol is a
        // prefix-coded byte string like any other, and that kernel decodes it once (symbol pool, byte path) where k_canon_decode
        // decodes it twice.  For tile shapes its byte path takes; what it leaves (GF_K_RETRY) k_canon_decode picks up.
        p.viaFast = !analysis && nRows >= 2 && nCols >= 4 && nCols <= 256 && cells + 8 <= p.fastM32;
        if (p.viaFast) {
            p.decThreads = lean ? 1024 : huffmanBuild(p.fastM32, 0);
            p.decBits |= gf_rt_dec_bit(4 /* DEC_FAST_CANON */, p.decThreads);
        }
        if (analysis) {
            p.decBits |= GF_RT_CANON_ANALYZE;                     // (the 256-thread build's LDS sizes)
        } else {
            // two builds as for the legacy decoder: 256 threads (up to five workgroups per CU) or 512 (four = 32 waves) ...
            GfDecodeArgs a{}, b{};
            a.ldsTextBytes = gf_canon_decode_lds_text(nRows, nCols);
            a.ldsStageBytes = gf_canon_decode_lds_stage(nRows, nCols);
            b.ldsTextBytes = gf_canon_decode_lds_text_t512(nRows, nCols);
            b.ldsStageBytes = gf_canon_decode_lds_stage_t512(nRows, nCols);
            const size_t waves256 = 4 * decWgsPerCu(gf_canon_decode_lds_per_wg(a), 8), waves512 = 8 * decWgsPerCu(gf_canon_decode_lds_per_wg_t512(b), 4);
            // ... where the tile is large enough to give most threads a subsequence (at least 128 bits each).  With the fused Triangle
            // inverse and the whole stream staged (late round 3) the 512-thread build wins from about 7,000 cells on: 90x120 tiles
            // 1.69 -> 1.37 ms per 16,000 tiles, 100x110 1.74 -> 1.40, 70x100 2.24 -> 2.22 per 33,000, 64x64 the same either way
            // (before those two: 70x100 2.50 with 256 threads against 2.81 with 512, and the bound was 12,000 cells)
#ifndef GF_CANON_T512_MIN_CELLS
#define GF_CANON_T512_MIN_CELLS 7000
#endif
            p.canonThreads = 2 * waves512 >= 3 * waves256 && cells >= GF_CANON_T512_MIN_CELLS ? 512 : 256;
            p.decBits |= p.canonThreads == 512 ? GF_RT_CANON_DEC_T512 : GF_RT_CANON_DEC_T256;
        }
        return GF_OK;
    }
    p.decThreads = huffmanBuild(p.fastM32, gf_huffman_decode_lds_text(nRows, nCols));
#ifdef GF_DEC_LDS_PAD_ENV
    if (const char *e = getenv("GF_DEC_FORCE_THREADS")) p.decThreads = atoi(e);   // experiment builds only (tools/occupancy_sweep.sh)
#endif
    if (lean) p.decThreads = 1024;
    if (kind == KIND_RAW_M32) {
        p.decBits = gf_rt_dec_bit(0 /* DEC_GENERAL */, p.decThreads);
        return GF_OK;
    }
    // CodecHuffman: the tree pre-pass, then (analysis) DEC_ANALYZE alone, or the fast kernel and the general one behind it
    p.prepass = (int32_t)gf_prepass_tiles_per_wave(nTiles);
    p.decBits = p.prepass == 1 ? GF_RT_TREES_1 : GF_RT_TREES_64;
    if (analysis) {
        p.decBits |= gf_rt_dec_bit(1 /* DEC_ANALYZE */, p.decThreads);
        return GF_OK;
    }
    p.decBits |= gf_rt_dec_bit(2 /* DEC_FAST */, p.decThreads);
    if (lean) return GF_OK;                                       // (the one-tile path: the fast kernel alone)
    p.decBits |= gf_rt_dec_bit(0 /* DEC_GENERAL */, p.decThreads);
    // the fast kernel runs twice: the usual LDS budget (1.125 M32 bytes per cell) and, for the tiles that outgrow it, two bytes
    // per cell; the pre-pass sorts the tiles
    const size_t roomy = std::min<size_t>(98304, (2 * cells + 1024 + 31) & ~(size_t)31);
    p.ldsM32Roomy = roomy > p.fastM32 ? (uint32_t)roomy : 0u;
    if (!p.ldsM32Roomy) return GF_OK;
    // The roomy run BESIDE the first run (round 5): it is a few hundred tiles of a rough batch at two workgroups per CU, a chain of
    // latencies that took 0.33 ms behind the first run's 1.2.  The roomy run stays on the caller's stream, directly behind the
    // pre-pass, and the FIRST run goes to the context's side stream: the roomy workgroups must reach the CUs first -- once four
    // workgroups of the first run hold a CU's LDS (4 x 40 KB), a 55 KB workgroup finds no room until two of them end together, i.e.
    // until the first run drains (measured: the other order gained 0.06 ms of the 0.33).
    // (a small batch -- BASELINE config 2: 1,024 tiles, 0.18 ms per decode -- loses more to the two hand-overs between the streams,
    // ~10 us each, than the roomy run could hide: 0.183 -> 0.201 ms measured; there the runs follow one another)
    // ... and a batch whose predecessors on this context listed no tile for the roomy run (smooth terrain: the run is 7 us of empty
    // workgroups) keeps everything on one stream: the hand-overs were 15-20 us of its 0.70 ms.  The hint (1 + the count of the
    // last batch whose general kernel has finished, 0 before the first) may be a batch or two old; either order of the runs is
    // correct for any data.
    const bool roomyLikely = roomySeen != 1u;
    const bool beside = side && nTiles >= 4096 && roomyLikely;
    // (round 6) a SMALL batch whose predecessors listed no tile for the roomy run does without its launch (5 us of BASELINE config
    // 2's 165): should the pre-pass list a tile after all, the first run tries it, the general kernel takes it, and the next batch
    // knows.  What a stale hint costs (measured on the rough surface with the launch left out of every batch below 4,096 tiles):
    // 1,024 tiles of 120 x 150 0.304 -> 0.339 ms, 1,300 0.350 -> 0.384, 3,000 0.530 -> 0.669 -- hence small batches only.  (For
    // every batch, with a reduced grid for the run where none is expected: a caller that queues a smooth batch and then rough ones
    // without waiting had each of them draw its 650 roomy tiles through 64 workgroups -- the default bench line's rough sub-record,
    // 1.37 -> 2.38 ms; taken back.)
    const bool noRoomy = !roomyLikely && nTiles < 2048;
    p.roomyForm = beside ? GF_ROOMY_BESIDE : noRoomy ? GF_ROOMY_SKIPPED : GF_ROOMY_BEHIND;
    if (p.roomyForm != GF_ROOMY_SKIPPED) p.decBits |= gf_rt_dec_bit(3 /* DEC_FAST_ROOMY */, p.decThreads);
    return GF_OK;
}

// ------------------------------------------------------------------ scratch plan
// What a batch needs of the context's three scratch buffers and where the parts lie (gvrs_api_internal.h).  No device, no HIP call.
// Exported for the tests as gf_internal_scratch_plan / gf_internal_scratch_reserve (loaded by name, like gf_internal_route_plan).
gf_status scratchPlan(int kind, int nRows, int nCols, size_t nTiles, int lean, int viaFast, gf_scratch_plan &p)
{
    p = gf_scratch_plan{};
    if (nRows < 1 || nCols < 1 || kind < KIND_HUFFMAN || kind > KIND_LSOP_ENC || kind == KIND_DEFLATE || kind == KIND_FLOAT) return GF_ERR_ARG;
    const size_t n = nTiles, cells = (size_t)nRows * (size_t)nCols, lengthBytes = n * GF_CANON_REC_WORDS * 4;
    if (kind != KIND_CANON && kind != KIND_LSOP_ENC) {
        // spill layout of the decode kernel: M32 bytes (6 per cell, rounded to 32), start bitmap, rank bases
        const size_t cap = roundUp(6 * cells, 32);
        p.wsStride = roundUp(cap + 2 * ((cap >> 5) + 2) * 4 + 64, 16);
        p.workspace = gf_huffman_decode_grid(n) * p.wsStride;
    }
    if (kind == KIND_HUFFMAN) p.leaf = {0, n * GF_TREE_REC_WORDS * 4}, p.spare = {p.leaf.bytes, 16}, p.roomy = {p.leaf.bytes + 16, n * 4};
    if (kind == KIND_CANON) p.lengths = {0, lengthBytes}, p.slack = {lengthBytes, 16 + (viaFast ? 4096u : 0u)};
    if (kind == KIND_LSOP_DEC) p.lsop0 = {0, lengthBytes}, p.lsop1 = {lengthBytes, lengthBytes};      // (both streams' records: k_lsop_head)
    p.trees = kind == KIND_LSOP_DEC ? 2 * lengthBytes + 16 : p.roomy.at + p.roomy.bytes + p.slack.at + p.slack.bytes;     // (one of the two at most)
    if (kind == KIND_LSOP_ENC) p.hist = {0, n * gf_lsop_hist_rec_words() * 4}, p.packRecs = p.hist.bytes + 16;
    if (kind == KIND_LSOP_ENC || kind == KIND_LSOP_DEC) return GF_OK;
    // the encoders' per-tile records between their kernels: selection records, behind them the statistics (CodecHuffman: what
    // k_huffman_encode hands to k_huffman_trees) and, at the next multiple of 256 bytes, the byte plane of raw row differences
    // (GfEncodeArgs::plane, round 6).  One size for both encoders: a context that writes with both never moves the buffer.
    const size_t huff = (size_t)GF_PACK_REC_WORDS + GF_ENC_STAT_WORDS, canon = gf_canon_pack_rec_words() + gf_canon_stat_words();
    const size_t planeStride = roundUp(cells, 16), selWords = kind == KIND_CANON ? gf_canon_pack_rec_words() : (size_t)GF_PACK_REC_WORDS;
    p.sel = {0, n * selWords * 4};
    p.stats = {p.sel.bytes, n * ((kind == KIND_CANON ? canon : huff) - selWords) * 4};
    if (!lean && kind != KIND_RAW_M32) p.planeStride = planeStride, p.plane = {roundUp(p.stats.at + p.stats.bytes + 16, 256), n * planeStride};
    p.packRecs = roundUp(n * std::max(huff, canon) * 4 + 16, 256) + n * planeStride + 256;
    return GF_OK;
}

void scratchReserve(int nRows, int nCols, size_t nTiles, uint64_t need[3])
{
    need[0] = need[1] = need[2] = 0;
    gf_scratch_plan p;
    for (int kind = KIND_HUFFMAN; kind <= KIND_LSOP_ENC; kind++)
        if (scratchPlan(kind, nRows, nCols, nTiles, 0, 1, p) == GF_OK)                // (viaFast: the larger of the two)
            need[0] = std::max(need[0], p.workspace), need[1] = std::max(need[1], p.trees), need[2] = std::max(need[2], p.packRecs);
}

// the launchers' report against the plan: a difference is a bug of this file, not of the data
static gf_status routeCheck(const char *what, uint32_t ran, uint32_t planned)
{
    if (ran == planned) return GF_OK;
    char buf[128];
    snprintf(buf, sizeof buf, "%s launched kernels 0x%x where the route plan has 0x%x", what, ran, planned);
    g_lastError = buf;
    return GF_ERR_HIP;
}

gf_status encodeBatchDev(int kind, gf_context *c, void *stream, int codecIndex, int nRows, int nCols, size_t nTiles,
                         const int32_t *dValues, uint8_t *dOut, size_t slotStride, uint32_t *dLengths, uint8_t *dPredictors,
                         int32_t *dStatus, int predictorMask, int lean)
{
    if (!c || nRows < 1 || nCols < 1 || !dValues || !dOut || !dLengths || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if ((size_t)nRows * (size_t)nCols >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    if (slotStride % 16 != 0 || ((uintptr_t)dOut & 15) != 0 || slotStride < 16) return GF_ERR_ARG;
    gf_route_plan plan{};                                   // (other kinds: the general encoder, no plan)
    if (kind == KIND_HUFFMAN || kind == KIND_CANON) {
        const gf_status s = routePlan(kind, nRows, nCols, nTiles, lean, 0, 0u, 0, plan);
        if (s != GF_OK) return s;
    }
    GfEncodeArgs a;
    a.values = dValues;
    a.out = dOut;
    a.lengths = dLengths;
    a.predictors = dPredictors;
    a.status = dStatus;
    a.nTiles = nTiles;
    a.slotStride = slotStride;
    a.nRows = nRows;
    a.nCols = nCols;
    a.codecIndex = codecIndex;
    a.predictorMask = predictorMask & GF_PM_ALL;
    a.debug = g_encodeDebug;
    a.phaseLimit = g_encPhaseLimit;
    a.retryFlag = kind == KIND_HUFFMAN ? (uint32_t *)c->flags.p + 4 : nullptr;      // (word 0 belongs to the decoder)
    gf_scratch_plan sp;
    if (gf_status s = scratchPlan(kind, nRows, nCols, nTiles, lean, 0, sp); s != GF_OK || (s = c->packRecs.ensure(sp.packRecs)) != GF_OK) return s;
    a.packRecs = c->packRecs.at<uint32_t>(sp.sel.at);
    a.lean = lean;
    a.encStats = c->packRecs.at<uint32_t>(sp.stats.at);
    a.planeStride = sp.planeStride;                        // (0 and no plane on the lean path)
    a.plane = sp.planeStride ? c->packRecs.at<uint8_t>(sp.plane.at) : nullptr;
    const hipStream_t st = streamOf(c, stream);
    uint32_t ran = 0;
    if (kind == KIND_CANON) GF_HIP(gf_launch_canon_encode(a, st, &ran));
    else if (plan.leanEncode)                                                           // one tile per call: the 1024-thread build
        GF_HIP(gf_launch_huffman_encode_lean_t1024(a, st, &ran));
    else GF_HIP(gf_launch_huffman_encode(a, st, &ran));
    c->routeEnc = ran;
    c->routeEncKind = kind;
    if ((kind == KIND_HUFFMAN || kind == KIND_CANON) && nTiles) return routeCheck("encode", ran, plan.encBits);
    return GF_OK;
}

gf_status decodeBatchDev(int kind, gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                         size_t blobBytes, const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues,
                         int32_t *dStatus, int lean, uint32_t *analysis, uint32_t *pairCounts)
{
    if (!c || nRows < 1 || nCols < 1 || !dBlob || !dLengths || !dValues || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if ((size_t)nRows * (size_t)nCols >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    if (((uintptr_t)dBlob & 3) != 0) return GF_ERR_ARG;
    // (the hint of GfDecodeArgs::roomySeenHost: read once, here, for the plan)
    const uint32_t roomySeen = c->hRoomySeen ? *(volatile const uint32_t *)c->hRoomySeen : 0u;
    gf_route_plan plan;
    {
        const gf_status s = routePlan(kind, nRows, nCols, nTiles, lean, analysis != nullptr, roomySeen, c->side.stream != nullptr, plan);
        if (s != GF_OK) return s;
    }
#ifdef GF_DIAG
    // (the diagnostic build's phase limits and cycle stamps are k_canon_decode's: tools/phase_cycles_canon.py, pmc_phases_canon.sh)
    if (kind == KIND_CANON && plan.viaFast && (g_decPhaseLimit || g_decodeDebug)) {
        plan.viaFast = 0;
        plan.decBits &= ~gf_rt_dec_bit(4 /* DEC_FAST_CANON */, plan.decThreads);
        plan.decThreads = 0;
    }
#endif
    const hipStream_t st = streamOf(c, stream);
    uint32_t ran = 0;
    const unsigned grid = gf_huffman_decode_grid(nTiles);
    // (neither ensure is capture-safe: callers that capture graphs call gf_context_reserve first)
    gf_scratch_plan sp;
    if (gf_status s = scratchPlan(kind, nRows, nCols, nTiles, lean, plan.viaFast, sp);
        s != GF_OK || (s = c->workspace.ensure(sp.workspace)) != GF_OK || (s = c->trees.ensure(sp.trees)) != GF_OK)
        return s;
    GfDecodeArgs a{};
    a.blob = dBlob;
    a.blobBytes = blobBytes;
    a.offsets = dOffsets;
    a.slotStride = slotStride;
    a.lengths = dLengths;
    a.values = dValues;
    a.status = dStatus;
    a.workspace = (uint8_t *)c->workspace.p;
    a.workspaceStride = sp.wsStride;
    a.nTiles = nTiles;
    a.nRows = nRows;
    a.nCols = nCols;
    a.phaseLimit = g_decPhaseLimit;
    a.debug = g_decodeDebug;
    a.rawM32 = kind == KIND_RAW_M32 ? 1 : 0;
    a.analysis = analysis;
    a.pairCounts = pairCounts;
    a.lean = lean;
    if (kind == KIND_HUFFMAN) {
        // tree pre-pass: one lane per tile walks the serialised tree; the decode kernel starts from the leaf records
        uint32_t *roomyList = c->trees.at<uint32_t>(sp.roomy.at);
        if (!analysis) a.retryFlag = (uint32_t *)c->flags.p;
        // (the fast kernel runs twice where the plan gives it a roomy run: the pre-pass sorts the tiles)
        const uint32_t roomyBytes = plan.ldsM32Roomy, fastBytes = roomyBytes ? plan.fastM32 : 0u;
        a.ldsM32Roomy = roomyBytes;
        GF_HIP(gf_launch_huffman_parse_trees(dBlob, blobBytes, dOffsets, slotStride, dLengths, (uint32_t *)c->trees.p, nTiles,
                                             st, a.retryFlag, fastBytes, roomyBytes, roomyList));
        if (nTiles) ran |= gf_prepass_tiles_per_wave(nTiles) == 1u ? GF_RT_TREES_1 : GF_RT_TREES_64;
        a.roomyList = roomyList;
        a.roomySeenHost = c->hRoomySeen;
        a.trees = (const uint32_t *)c->trees.p;
        a.flagsCleared = a.retryFlag ? 1 : 0;
    }
    if (kind == KIND_CANON) {
        // the same for the canonical decoder's code lengths, behind the canonical run of the fast kernel where the plan has one
        if (plan.viaFast) a.retryFlag = (uint32_t *)c->flags.p;
        GF_HIP(gf_launch_canon_parse_lengths(dBlob, blobBytes, dOffsets, slotStride, dLengths, (uint32_t *)c->trees.p, nTiles, 0,
                                             st, a.retryFlag));
        if (nTiles) ran |= gf_prepass_tiles_per_wave(nTiles) == 1u ? GF_RT_LENGTHS_1 : GF_RT_LENGTHS_64;
        a.trees = (const uint32_t *)c->trees.p;
        if (plan.viaFast) {
            GfDecodeArgs f = a;
            f.ldsM32Bytes = plan.fastM32;
            f.ldsTextBytes = 0;
            f.ldsM32Roomy = 0;
            const int threads = plan.decThreads;
            if (threads == 1024) GF_HIP(gf_launch_huffman_decode_canon_t1024(f, st, &ran));
            else if (threads == 512) GF_HIP(gf_launch_huffman_decode_canon_t512(f, st, &ran));
            else GF_HIP(gf_launch_huffman_decode_canon(f, st, &ran));
        }
    }
    if (kind == KIND_CANON && analysis) {
        // CodecCanonHuffman.analyze: the text of every tile (the 256-thread build) and its symbol statistics, records to analysis
        a.ldsM32Bytes = 0;
        a.ldsTextBytes = gf_canon_decode_lds_text(nRows, nCols);
        a.ldsStageBytes = gf_canon_decode_lds_stage(nRows, nCols);
        GF_HIP(gf_launch_canon_analyze(a, st));
        if (nTiles) ran |= GF_RT_CANON_ANALYZE;
    } else if (kind == KIND_CANON) {
        // two builds as for the legacy decoder below: 256 threads (up to five workgroups per CU) or 512 (four = 32 waves)
        a.ldsM32Bytes = 0;
        GfDecodeArgs b = a;
        a.ldsTextBytes = gf_canon_decode_lds_text(nRows, nCols);
        a.ldsStageBytes = gf_canon_decode_lds_stage(nRows, nCols);
        b.ldsTextBytes = gf_canon_decode_lds_text_t512(nRows, nCols);
        b.ldsStageBytes = gf_canon_decode_lds_stage_t512(nRows, nCols);
        // (the build: routePlan)
        if (plan.canonThreads == 512) {
            GF_HIP(gf_launch_canon_decode_t512(b, st, grid));
            if (nTiles) ran |= GF_RT_CANON_DEC_T512;
        } else {
            GF_HIP(gf_launch_canon_decode(a, st, grid));
            if (nTiles) ran |= GF_RT_CANON_DEC_T256;
        }
    } else {
        a.ldsM32Bytes = gf_huffman_decode_lds_m32(nRows, nCols);
        a.ldsTextBytes = gf_huffman_decode_lds_text(nRows, nCols);
        // the build and the roomy run's form: routePlan
        const int threads = plan.decThreads;
        const GfSideStream *side = c->side.stream ? &c->side : nullptr;
        const int form = plan.roomyForm;
        if (threads == 1024) GF_HIP(gf_launch_huffman_decode_t1024(a, st, grid, side, form, &ran));
        else if (threads == 512) GF_HIP(gf_launch_huffman_decode_t512(a, st, grid, side, form, &ran));
        else GF_HIP(gf_launch_huffman_decode(a, st, grid, side, form, &ran));
    }
    c->routeDec = ran;
    c->routeDecKind = kind;
    c->routeRoomy = plan.roomyForm;
    c->routePrepass = plan.prepass;
    return nTiles ? routeCheck("decode", ran, plan.decBits) : GF_OK;
}

extern "C" {

// Not part of the public ABI (tests load them by name; include/gvrs_hip_codec.h and _lib.SIGNATURES do not list them).
// gf_internal_route_plan: routePlan for a context that has its side stream.  No device is needed.
gf_status gf_internal_route_plan(int kind, int nRows, int nCols, size_t nTiles, int lean, int analysis, uint32_t roomySeen,
                                 gf_route_plan *out)
{
    if (!out) return GF_ERR_ARG;
    return routePlan(kind, nRows, nCols, nTiles, lean, analysis, roomySeen, 1, *out);
}
size_t gf_internal_route_plan_bytes(void) { return sizeof(gf_route_plan); }
// scratchPlan and scratchReserve (need: workspace, trees, packRecs).  No device is needed.
gf_status gf_internal_scratch_plan(int kind, int nRows, int nCols, size_t nTiles, int lean, int viaFast, gf_scratch_plan *out)
{
    return out ? scratchPlan(kind, nRows, nCols, nTiles, lean, viaFast, *out) : GF_ERR_ARG;
}
size_t gf_internal_scratch_plan_bytes(void) { return sizeof(gf_scratch_plan); }
gf_status gf_internal_scratch_reserve(int nRows, int nCols, size_t nTiles, uint64_t need[3])
{
    if (!need || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    scratchReserve(nRows, nCols, nTiles, need);
    return GF_OK;
}
// LDS bytes per workgroup (static + dynamic) that the plan weighs: build 0, 1, 2 = k_huffman_decode with 256, 512, 1024 threads
// at the given M32 and text capacities; 3, 4 = k_canon_decode with 256, 512 threads at its own sizes for the tile shape
size_t gf_internal_decode_lds_per_wg(int build, int nRows, int nCols, uint32_t ldsM32, uint32_t ldsText)
{
    GfDecodeArgs a{};
    a.ldsM32Bytes = ldsM32;
    a.ldsTextBytes = ldsText;
    switch (build) {
    case 0: return gf_huffman_decode_lds_per_wg(a);
    case 1: return gf_huffman_decode_lds_per_wg_t512(a);
    case 2: return gf_huffman_decode_lds_per_wg_t1024(a);
    case 3:
        a.ldsTextBytes = gf_canon_decode_lds_text(nRows, nCols);
        a.ldsStageBytes = gf_canon_decode_lds_stage(nRows, nCols);
        return gf_canon_decode_lds_per_wg(a);
    case 4:
        a.ldsTextBytes = gf_canon_decode_lds_text_t512(nRows, nCols);
        a.ldsStageBytes = gf_canon_decode_lds_stage_t512(nRows, nCols);
        return gf_canon_decode_lds_per_wg_t512(a);
    default: return 0;
    }
}

// What the context's last encode and last decode batch launched, from host-side records of the launch sites.  The device words
// (the retry words of c->flags and the roomy hint) are copied back here, so call it after synchronising the context's streams:
// nothing of this is read on the batch path.
struct gf_route_report {
    uint32_t encBits, decBits;      // GF_RT_* of the last encode / decode batch
    int32_t encKind, decKind;       // their codec kinds (KIND_*), -1 before the first
    int32_t roomyForm, prepass;     // the last decode batch's GF_ROOMY_* and pre-pass tiles per wave
    uint32_t roomySeen;             // GfDecodeArgs::roomySeenHost: 1 + the tiles the pre-pass listed for the roomy run (0: none yet)
    uint32_t pad;
    uint32_t flags[8];              // c->flags: decode retry words 0 and 1 (GfDecodeArgs::retryFlag), roomy count and cursor 2 and 3;
                                    // encode retry words 4 and 5 (GfEncodeArgs::retryFlag: 5 counts the tiles left to k_huffman_pack_rare)
};
gf_status gf_internal_route_report(gf_context *c, gf_route_report *out)
{
    GF_CTX_LOCK(c);
    if (!c || !out) return GF_ERR_ARG;
    gf_route_report r{};
    r.encBits = c->routeEnc;
    r.decBits = c->routeDec;
    r.encKind = c->routeEncKind;
    r.decKind = c->routeDecKind;
    r.roomyForm = c->routeRoomy;
    r.prepass = c->routePrepass;
    r.roomySeen = c->hRoomySeen ? *(volatile const uint32_t *)c->hRoomySeen : 0u;
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(hipMemcpy(r.flags, c->flags.p, sizeof r.flags, hipMemcpyDeviceToHost));
    *out = r;
    return GF_OK;
}
size_t gf_internal_route_report_bytes(void) { return sizeof(gf_route_report); }

gf_status gf_huffman_encode_batch_i32_dev(gf_context *c, void *stream, int codecIndex, int nRows, int nCols,
                                          size_t nTiles, const int32_t *dValues, uint8_t *dOut, size_t slotStride,
                                          uint32_t *dLengths, uint8_t *dPredictors, int32_t *dStatus,
                                          int predictorMask)
{
    GF_CTX_LOCK(c);
    return encodeBatchDev(KIND_HUFFMAN, c, stream, codecIndex, nRows, nCols, nTiles, dValues, dOut, slotStride, dLengths,
                          dPredictors, dStatus, predictorMask, 0);
}

gf_status gf_huffman_decode_batch_i32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles,
                                          const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                                          size_t slotStride, const uint32_t *dLengths, int32_t *dValues,
                                          int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    return decodeBatchDev(KIND_HUFFMAN, c, stream, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths,
                          dValues, dStatus, 0);
}

gf_status gf_canon_encode_batch_i32_dev(gf_context *c, void *stream, int codecIndex, int nRows, int nCols,
                                        size_t nTiles, const int32_t *dValues, uint8_t *dOut, size_t slotStride,
                                        uint32_t *dLengths, uint8_t *dPredictors, int32_t *dStatus, int predictorMask)
{
    GF_CTX_LOCK(c);
    return encodeBatchDev(KIND_CANON, c, stream, codecIndex, nRows, nCols, nTiles, dValues, dOut, slotStride, dLengths,
                          dPredictors, dStatus, predictorMask, 0);
}

gf_status gf_canon_decode_batch_i32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles,
                                        const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                                        size_t slotStride, const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    return decodeBatchDev(KIND_CANON, c, stream, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths,
                          dValues, dStatus, 0);
}

size_t gf_canon_max_packing(int nRows, int nCols)
{
    // 6 header bytes + code tables (< 750 bytes) + per value at most 4 symbols of 15 bits and 24 raw bits + end-of-text
    const size_t cells = (size_t)nRows * (size_t)nCols;
    return roundUp(6 + 768 + (cells * 84 + 15 + 7) / 8 + 16, 16);
}

gf_status gf_compact_dev(gf_context *c, void *stream, size_t nTiles, const uint8_t *dSlots, size_t slotStride,
                         const uint32_t *dLengths, uint64_t *dOffsets, uint8_t *dBlob, size_t blobCap)
{
    GF_CTX_LOCK(c);
    if (!c || !dSlots || !dLengths || !dOffsets || !dBlob) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if (((uintptr_t)dSlots & 15) != 0 || slotStride % 16 != 0) return GF_ERR_ARG;
    GF_HIP(gf_launch_compact(nTiles, dSlots, slotStride, dLengths, dOffsets, dBlob, blobCap,
                             streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_synth_dem_dev(gf_context *c, void *stream, uint64_t seed, int nRows, int nCols, int64_t tilesPerRow,
                           int64_t tile0, size_t nTiles, int32_t *dValues)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || tilesPerRow < 1 || !dValues) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    GF_HIP(gf_launch_synth_dem(seed, nRows, nCols, tilesPerRow, tile0, nTiles, dValues,
                               streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_synth_dem_masked_dev(gf_context *c, void *stream, uint64_t seed, int nRows, int nCols, int64_t tilesPerRow,
                                  int64_t tile0, size_t nTiles, int maskPerMille, int32_t *dValues)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || tilesPerRow < 1 || !dValues || maskPerMille < 0 || maskPerMille > 1000) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(gf_launch_synth_dem(seed, nRows, nCols, tilesPerRow, tile0, nTiles, dValues,
                               streamOf(c, stream), maskPerMille));
    return GF_OK;
}

gf_status gf_synth_dem_style_dev(gf_context *c, void *stream, uint64_t seed, int nRows, int nCols, int64_t tilesPerRow,
                                 int64_t tile0, size_t nTiles, int maskPerMille, int style, int32_t *dValues)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || tilesPerRow < 1 || !dValues || maskPerMille < 0 || maskPerMille > 1000) return GF_ERR_ARG;
    if (style != GF_DEM_STYLE_CLASSIC && style != GF_DEM_STYLE_ROUGH) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(gf_launch_synth_dem(seed, nRows, nCols, tilesPerRow, tile0, nTiles, dValues,
                               streamOf(c, stream), maskPerMille, style));
    return GF_OK;
}

// ---- M32 streams: the device stage of CodecDeflate (gvrs_api_deflate.hip)

gf_status gf_m32_encode_batch_i32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const int32_t *dValues,
                                      uint8_t *dStreams, size_t subStride, uint32_t *dLengths, uint8_t *dModels,
                                      uint32_t *dSeeds, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !dValues || !dStreams || !dLengths || !dModels || !dSeeds || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if ((size_t)nRows * (size_t)nCols >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    if (subStride % 16 != 0 || subStride < 16 || ((uintptr_t)dStreams & 15) != 0) return GF_ERR_ARG;
    GfM32Args a;
    a.values = dValues;
    a.out = dStreams;
    a.subStride = subStride;
    a.lengths = dLengths;
    a.models = dModels;
    a.seeds = dSeeds;
    a.status = dStatus;
    a.nTiles = nTiles;
    a.nRows = nRows;
    a.nCols = nCols;
    GF_HIP(gf_launch_m32_streams(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_m32_decode_batch_i32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                                      size_t blobBytes, const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths,
                                      int32_t *dValues, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    return decodeBatchDev(KIND_RAW_M32, c, stream, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths,
                          dValues, dStatus, 0);
}

}  // extern "C"
