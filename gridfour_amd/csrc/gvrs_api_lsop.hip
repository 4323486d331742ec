// gvrs_api_lsop.hip -- LSOP12 and LSOP08: the device-resident and the host-memory entry points.

#include "gvrs_api_internal.h"

// code-length pre-pass for the first stream of LSOP12 containers of the canonical type (the caller has checked c and set its device)
static gf_status lsopParseLengths(gf_context *c, hipStream_t st, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                                  const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, gf_scratch_plan &sp)
{
    gf_status s = scratchPlan(KIND_LSOP_DEC, 1, 1, nTiles, 0, 0, sp);             // (the records do not depend on the tile shape)
    if (s != GF_OK || (s = c->trees.ensure(sp.trees)) != GF_OK) return s;
    GF_HIP(gf_launch_canon_parse_lengths(dBlob, blobBytes, dOffsets, slotStride, dLengths, c->trees.at<uint32_t>(sp.lsop0.at), nTiles, 1, st));
    return GF_OK;
}

// second entropy pass of the LSOP12 decode: containers k_lsop_unpack2 left marked GF_ERR_UNSUPPORTED (legacy Huffman of
// M32; with rawM32 also the host-inflated Deflate ones)
static gf_status lsopUnpackM32(gf_context *c, hipStream_t st, const GfLsopForm &form, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                               size_t blobBytes, const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths,
                               int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus, int rawM32,
                               const uint8_t *rawSide = nullptr, size_t rawSideStride = 0, const int32_t *sideStatus = nullptr,
                               const uint32_t *produced2 = nullptr, const int32_t *inflStatus2 = nullptr)
{
    const unsigned grid = gf_huffman_decode_grid(nTiles);
    gf_scratch_plan sp;
    gf_status s = scratchPlan(KIND_LSOP_DEC, nRows, nCols, nTiles, 0, 0, sp);
    if (s != GF_OK || (s = c->workspace.ensure(sp.workspace)) != GF_OK) return s;
    GfLsopM32Args a;
    a.blob = dBlob;
    a.blobBytes = blobBytes;
    a.offsets = dOffsets;
    a.slotStride = slotStride;
    a.lengths = dLengths;
    a.residuals = dResiduals;
    a.resStride = resStride;
    a.coefs = dCoefs;
    a.status = dScratchStatus;
    a.workspace = (uint8_t *)c->workspace.p;
    a.workspaceStride = sp.wsStride;
    a.nTiles = nTiles;
    a.nRows = nRows;
    a.nCols = nCols;
    a.ldsM32Bytes = gf_huffman_decode_lds_m32(nRows, nCols);
    a.rawM32 = rawM32;
    a.rawSide = rawSide;
    a.rawSideStride = rawSideStride;
    a.sideStatus = sideStatus;
    a.produced2 = produced2;
    a.inflStatus2 = inflStatus2;
    a.form = form;
    GF_HIP(gf_launch_lsop_unpack_m32(a, st, grid));
    return GF_OK;
}

constexpr size_t LSOP_INFLATE_SCRATCH_BYTES = (size_t)384 << 20;   // LSOP12's Deflate containers (rare: see lsopUnpackM32Deflate)

// Second entropy pass of the LSOP12 decode with the Deflate containers inflated ON THE DEVICE (LsDecoder12.java:127-141):
// per chunk of tiles, k_lsop_streams describes the first zlib stream of every Deflate container, k_inflate runs, k_lsop_streams
// places the second stream behind what the first one consumed, k_inflate runs again, and k_lsop_unpack_m32 reads the M32 bytes
// of those tiles from the scratch (legacy Huffman containers are decoded as stored in the same launch).
static gf_status lsopUnpackM32Deflate(gf_context *c, hipStream_t st, const GfLsopForm &form, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                                      size_t blobBytes, const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths,
                                      int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus)
{
    const size_t nInit = form.nInit, nInt = form.nInt;
    const size_t rawStride = roundUp(6 * (nInit + nInt) + 192, 16);
    // The scratch of the Deflate containers: LSOP_INFLATE_SCRATCH_BYTES, not a share of HBM per tile of the batch -- the default
    // encoder output is the canonical container and pays these gated launches for nothing (the full gigabyte of the CodecDeflate /
    // CodecFloat paths made a gigabyte of every context -- read-ahead, gf_multi shards -- that ever decoded an LSOP tile)
    const size_t chunk = std::max<size_t>(1, std::min(nTiles, LSOP_INFLATE_SCRATCH_BYTES / rawStride));
    gf_status s;
    if ((s = c->dInflOut.ensure(chunk * rawStride + 64)) != GF_OK) return s;
    if ((s = c->dInflate.ensure(chunk * sizeof(GfInflateStream))) != GF_OK) return s;
    Carve k;
    size_t at[6];                            // per stream: produced, consumed, produced (second stream), the two statuses, the side table
    for (size_t &x : at) x = k.add(chunk * 4);
    const size_t gateAt = k.add(4);
    if ((s = c->dInflMeta.ensure(k, chunk * 4 + 112)) != GF_OK) return s;
    uint8_t *raw = (uint8_t *)c->dInflOut.p;
    GfInflateStream *desc = (GfInflateStream *)c->dInflate.p;
    uint32_t *produced1 = c->dInflMeta.at<uint32_t>(at[0]), *consumed1 = c->dInflMeta.at<uint32_t>(at[1]), *produced2 = c->dInflMeta.at<uint32_t>(at[2]);
    int32_t *status1 = c->dInflMeta.at<int32_t>(at[3]), *status2 = c->dInflMeta.at<int32_t>(at[4]), *side = c->dInflMeta.at<int32_t>(at[5]);
    uint32_t *gate = c->dInflMeta.at<uint32_t>(gateAt);            // number of Deflate containers in the chunk
    for (size_t t0 = 0; t0 < nTiles; t0 += chunk) {
        const size_t n = std::min(chunk, nTiles - t0);
        GF_HIP(hipMemsetAsync(gate, 0, 4, st));
        // this chunk's view of the batch
        const uint8_t *blobC = dOffsets ? dBlob : dBlob + t0 * slotStride;
        const size_t blobBytesC = dOffsets ? blobBytes : blobBytes - t0 * slotStride;
        const uint64_t *offC = dOffsets ? dOffsets + t0 : nullptr;
        for (int pass = 0; pass < 2; pass++) {
            GF_HIP(gf_launch_lsop_streams(blobC, blobBytesC, offC, slotStride, dLengths + t0, n, form, rawStride,
                                          pass, produced1, status1, consumed1, desc, side, gate, st));
            GfInflateArgs a{};
            a.inBase = blobC;
            a.outBase = raw;
            a.streams = desc;
            a.produced = pass ? produced2 : produced1;
            a.status = pass ? status2 : status1;
            a.consumed = pass ? nullptr : consumed1;
            a.gate = gate;
            a.nStreams = n;
            a.window = gf_inflate_window(0);
            GF_HIP(gf_launch_inflate(a, st));
        }
        s = lsopUnpackM32(c, st, form, nRows, nCols, n, blobC, blobBytesC, offC, slotStride, dLengths + t0, dResiduals + t0 * resStride, resStride,
                          dCoefs + t0 * 16, dScratchStatus + t0, 2, raw, rawStride, side, produced2, status2);
        if (s != GF_OK) return s;
    }
    return GF_OK;
}

// (round 6, advice) int32Residuals: the caller reads d_residuals itself (gf_lsop12_encode_batch_i32's Deflate stage) -- a parameter of
// this internal form, no longer an undocumented bit of the public flags word
static gf_status lsopEncodeBatchDev(gf_context *c, void *stream, int codecIndex, int nRows, int nCols, size_t nTiles,
                                    const int32_t *dValues, int flags, bool int32Residuals, uint8_t *dOut, size_t slotStride,
                                    uint32_t *dLengths, int32_t *dStatus, int32_t *dResiduals, size_t resStride, uint32_t *dCoefs,
                                    int32_t *dScratchStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dOut || !dLengths || !dStatus || !dResiduals || !dCoefs || !dScratchStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if (slotStride % 16 != 0 || ((uintptr_t)dOut & 15) != 0 || slotStride < 64) return GF_ERR_ARG;
    const hipStream_t st = streamOf(c, stream);
    if (nRows < 6 || nCols < 6) {
        if (nTiles) {
            GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, st));
            GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dLengths, 0, nTiles, st));
        }
        return GF_OK;
    }
    // Terrain-sized tiles (round 5): the first kernel keeps the tile in LDS as halfwords, writes the residuals as int16 and counts
    // the histograms on the way (k_lsop_predict16; records in the context's selection-record buffer, which gf_context_reserve
    // sizes) -- unless the caller wants the int32 residuals themselves (int32Residuals: the host's Deflate stage)
    const bool fast16 = gf_lsop_predict16_eligible(nRows, nCols) && !int32Residuals && resStride >= gf_lsop12_residual_count(nRows, nCols);
    uint32_t *hist16 = nullptr;
    gf_status s;
    if (fast16) {
        gf_scratch_plan sp;
        if ((s = scratchPlan(KIND_LSOP_ENC, nRows, nCols, nTiles, 0, 0, sp)) != GF_OK || (s = c->packRecs.ensure(sp.packRecs)) != GF_OK) return s;
        hist16 = c->packRecs.at<uint32_t>(sp.hist.at);
        GF_HIP(gf_launch_lsop_predict16(dValues, dResiduals, resStride, dCoefs, dScratchStatus, hist16, nTiles, nRows, nCols, st));
    } else {
        s = gf_lsop12_predict_dev(c, stream, nRows, nCols, nTiles, dValues, dResiduals, resStride, dCoefs, dScratchStatus);
        if (s != GF_OK) return s;
    }
    const uint32_t n0 = (uint32_t)(4 * nRows + 2 * nCols - 9), n1 = (uint32_t)((nRows - 2) * (nCols - 4));
    if (4ull * ((uint64_t)n1 + 1) >= (1ull << 22)) return GF_ERR_UNSUPPORTED;       // 22-bit counts in the tree keys
    const int valueChecksum = (flags & GF_LSOP_VALUE_CHECKSUM) ? 1 : 0;
    if (valueChecksum)
        GF_HIP(gf_launch_lsop_value_crc(dValues, (size_t)nRows * (size_t)nCols, nTiles, nullptr, dCoefs, st));
    GF_HIP(gf_launch_canon_pack2(dResiduals, resStride, dCoefs, dScratchStatus, dOut, slotStride, dLengths, dStatus, nTiles,
                                 n0, n1, codecIndex, st, valueChecksum, hist16));
    return GF_OK;
}

// CodecM32.encode (compress/CodecM32.java:257-311) of a residual array: host-side glue for the Deflate container
static size_t m32Pack(const int32_t *x, size_t n, std::vector<uint8_t> &out)
{
    out.resize(6 * n + 8);
    size_t k = 0;
    for (size_t i = 0; i < n; i++) {
        const int len = gf_m32_len((uint32_t)x[i]);
        for (int b = 0; b < len; b++) out[k++] = (uint8_t)gf_m32_byte((uint32_t)x[i], len, b);
    }
    out.resize(k);
    return k;
}

extern "C" {

// ------------------------------------------------------------------ LSOP12

size_t gf_lsop12_residual_count(int nRows, int nCols)
{
    if (nRows < 6 || nCols < 6) return 0;
    return (size_t)4 * nRows + (size_t)2 * nCols - 9 + (size_t)(nRows - 2) * (size_t)(nCols - 4);
}

size_t gf_lsop12_max_packing(int nRows, int nCols)
{
    // 55 header bytes (59 with the value checksum) + two canonical-Huffman streams (tables < 750 bytes each, at most 84 bits per
    // value + end-of-text)
    const size_t n = gf_lsop12_residual_count(nRows, nCols);
    return roundUp(59 + 2 * 768 + (n * 84 + 2 * 15 + 7) / 8 + 16, 16);
}

gf_status gf_lsop12_predict_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const int32_t *dValues,
                                int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dResiduals || !dCoefs || !dStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if ((size_t)nRows * (size_t)nCols >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    const hipStream_t st = streamOf(c, stream);
    if (nRows < 6 || nCols < 6) {                       // LsOptimalPredictor12.java:114-116 -> null
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, st));
        return GF_OK;
    }
    if (resStride < gf_lsop12_residual_count(nRows, nCols)) return GF_ERR_ARG;
    GF_HIP(gf_launch_lsop_predict(dValues, dResiduals, resStride, dCoefs, dStatus, nTiles, nRows, nCols, st));
    return GF_OK;
}

gf_status gf_lsop12_reconstruct_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles,
                                    const int32_t *dResiduals, size_t resStride, const uint32_t *dCoefs,
                                    const int32_t *dInStatus, int32_t *dValues, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dResiduals || !dCoefs || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if (nRows < 6 || nCols < 6 || resStride < gf_lsop12_residual_count(nRows, nCols)) return GF_ERR_ARG;
    // planes: word GF_LSOP_FMT_WORD says how a tile's interior residuals lie -- 0 in a record the caller built (the ABI asks for
    // words 13 .. 15 = 0) or one gf_lsop12_predict_dev wrote, 1 for a byte plane gf_lsop12_decode_batch_i32_dev left
    GF_HIP(gf_launch_lsop_reconstruct(dResiduals, resStride, dCoefs, dInStatus, dValues, dStatus, nTiles, nRows, nCols,
                                      streamOf(c, stream), true));
    return GF_OK;
}

gf_status gf_lsop12_encode_batch_i32_dev(gf_context *c, void *stream, int codecIndex, int nRows, int nCols, size_t nTiles,
                                         const int32_t *dValues, uint8_t *dOut, size_t slotStride, uint32_t *dLengths,
                                         int32_t *dStatus, int32_t *dResiduals, size_t resStride, uint32_t *dCoefs,
                                         int32_t *dScratchStatus)
{
    return gf_lsop12_encode_batch_i32_dev_ex(c, stream, codecIndex, nRows, nCols, nTiles, dValues, 0, dOut, slotStride, dLengths, dStatus,
                                             dResiduals, resStride, dCoefs, dScratchStatus);
}

// ... with LsEncoder12's switches (flags: GF_LSOP_VALUE_CHECKSUM = setValueChecksumEnabled, lsop/LsEncoder12.java:117-119; the
// Deflate alternative needs the host's zlib and is not a device-resident operation: GF_LSOP_DEFLATE is accepted and means nothing
// here; any other bit is GF_ERR_ARG)
gf_status gf_lsop12_encode_batch_i32_dev_ex(gf_context *c, void *stream, int codecIndex, int nRows, int nCols, size_t nTiles,
                                            const int32_t *dValues, int flags, uint8_t *dOut, size_t slotStride, uint32_t *dLengths,
                                            int32_t *dStatus, int32_t *dResiduals, size_t resStride, uint32_t *dCoefs,
                                            int32_t *dScratchStatus)
{
    if (flags & ~(GF_LSOP_DEFLATE | GF_LSOP_VALUE_CHECKSUM)) return GF_ERR_ARG;
    return lsopEncodeBatchDev(c, stream, codecIndex, nRows, nCols, nTiles, dValues, flags, false, dOut, slotStride, dLengths, dStatus,
                              dResiduals, resStride, dCoefs, dScratchStatus);
}

gf_status gf_lsop12_decode_batch_i32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles,
                                         const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets, size_t slotStride,
                                         const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus, int32_t *dResiduals,
                                         size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dBlob || !dLengths || !dValues || !dStatus || !dResiduals || !dCoefs || !dScratchStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if (((uintptr_t)dBlob & 3) != 0) return GF_ERR_ARG;
    const hipStream_t st = streamOf(c, stream);
    if (nRows < 6 || nCols < 6) {
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_ERR_BOUNDS, nTiles, st));
        return GF_OK;
    }
    if (resStride < gf_lsop12_residual_count(nRows, nCols)) return GF_ERR_ARG;
    const unsigned grid = gf_huffman_decode_grid(nTiles);
    gf_scratch_plan sp;
    gf_status s = lsopParseLengths(c, st, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths, sp);
    if (s != GF_OK) return s;
    // (round 6) interior residuals as byte planes in the reconstruction's order where a tile's values allow (gvrs_kernels.h)
    GF_HIP(gf_launch_lsop_unpack2(dBlob, blobBytes, dOffsets, slotStride, dLengths, dResiduals, resStride, dCoefs,
                                  dScratchStatus, nTiles, nRows, nCols, gf_lsop_unpack_lds_text(nRows, nCols), grid, st,
                                  c->trees.at<const uint32_t>(sp.lsop0.at), g_decodeDebug,
                                  // (the serial walk of a lane pays where sixty-four tiles share a wave: large batches)
                                  gf_prepass_tiles_per_wave(nTiles) == 64u ? c->trees.at<uint32_t>(sp.lsop1.at) : nullptr,
                                  true));
    s = lsopUnpackM32Deflate(c, st, gf_lsop12_form(nRows, nCols), nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths, dResiduals, resStride,
                             dCoefs, dScratchStatus);
    if (s != GF_OK) return s;
    GF_HIP(gf_launch_lsop_reconstruct(dResiduals, resStride, dCoefs, dScratchStatus, dValues, dStatus, nTiles, nRows, nCols, st,
                                      true));
    return GF_OK;
}

// LsEncoder12.encode :122-219 for a batch in host memory.  deflateEnabled mirrors setDeflateEnabled (default true):
// the canonical-Huffman packing comes from the GPU; with Deflate enabled the host's zlib (level 6) compresses the two
// M32 streams and replaces the packing when strictly smaller (:180-216).  types[t] = container type written (2 / 1).
gf_status gf_lsop12_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                     int deflateEnabled, uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *types,
                                     int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    if (deflateEnabled & ~(GF_LSOP_DEFLATE | GF_LSOP_VALUE_CHECKSUM)) return GF_ERR_ARG;      // (a bit mask since round 5: see the header)
    GF_HIP(hipSetDevice(c->device));
    if (nRows < 6 || nCols < 6) {
        for (size_t t = 0; t <= nTiles; t++) offsets[t] = 0;
        for (size_t t = 0; t < nTiles; t++) { if (status) status[t] = GF_DECLINED; if (types) types[t] = 0; }
        return GF_OK;
    }
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t nRes = gf_lsop12_residual_count(nRows, nCols), resStride = roundUp(nRes, 4);
    const size_t nInit = (size_t)4 * nRows + 2 * nCols - 9, nInt = nRes - nInit;
    const size_t stride = gf_lsop12_max_packing(nRows, nCols);
    // deflateEnabled carries LsEncoder12's two switches as bits: GF_LSOP_DEFLATE (setDeflateEnabled) and GF_LSOP_VALUE_CHECKSUM
    // (setValueChecksumEnabled); any other bit was refused above
    const bool valueChecksum = (deflateEnabled & GF_LSOP_VALUE_CHECKSUM) != 0;
    deflateEnabled &= GF_LSOP_DEFLATE;
    const size_t hdrCanon = valueChecksum ? 59 : 55, hdrDeflate = valueChecksum ? 67 : 63;
    // staging: values | slots | lengths | statuses | residuals | coefficients (the two come home for the host's Deflate alone) | the
    // second status
    std::vector<uint32_t> lengths(nTiles), coefs(deflateEnabled ? nTiles * 16 : 0);
    std::vector<int32_t> st(nTiles), res(deflateEnabled ? nTiles * resStride : 0);
    std::vector<uint8_t> slots(nTiles * stride);
    HostStage sg(c);
    const int valuesP = sg.in(values, nTiles * cells * 4), slotsP = sg.out(slots.data(), nTiles * stride);
    const int lengthsP = sg.out(lengths.data(), nTiles * 4), statusP = sg.out(st.data(), nTiles * 4);
    const int resP = deflateEnabled ? sg.out(res.data(), nTiles * resStride * 4) : sg.local(nTiles * resStride * 4);
    const int coefsP = deflateEnabled ? sg.out(coefs.data(), nTiles * 64) : sg.local(nTiles * 64);
    const int status2P = sg.local(nTiles * 4);
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    s = lsopEncodeBatchDev(c, c->stream, codecIndex, nRows, nCols, nTiles, sg.ptr<int32_t>(valuesP), valueChecksum ? GF_LSOP_VALUE_CHECKSUM : 0,
                           deflateEnabled != 0, sg.ptr<uint8_t>(slotsP), stride, sg.ptr<uint32_t>(lengthsP), sg.ptr<int32_t>(statusP),
                           sg.ptr<int32_t>(resP), resStride, sg.ptr<uint32_t>(coefsP), sg.ptr<int32_t>(status2P));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;

    std::vector<std::vector<uint8_t>> alt(nTiles);          // Deflate container where it wins
    if (deflateEnabled) {
        parallelFor(nTiles, [&](size_t t) {
            if (st[t] != GF_OK) return;
            const size_t canonLength = lengths[t] - hdrCanon;
            const int32_t *r = res.data() + t * resStride;
            std::vector<uint8_t> mInt, mInit, zInt, zInit;
            const size_t nMX = m32Pack(r + nInit, nInt, mInt);
            if (!zDeflate(mInt.data(), nMX, 6, zInt)) return;
            if (zInt.empty() || zInt.size() >= canonLength || zInt.size() > nMX + 128) return;      // :185-187
            const size_t nMI = m32Pack(r, nInit, mInit);
            if (!zDeflate(mInit.data(), nMI, 6, zInit)) return;
            if (zInit.empty() || zInit.size() + zInt.size() >= canonLength || zInit.size() > nMI + 128) return;   // :194-196
            std::vector<uint8_t> &p = alt[t];
            p.resize(hdrDeflate + zInit.size() + zInt.size());
            p[0] = (uint8_t)codecIndex;
            p[1] = valueChecksum ? 0xC1 : 0x41;              // COMPRESSION_TYPE_DEFLATE | REVISION_FLAG (| VALUE_CHECKSUM_INCLUDED)
            p[2] = 12;
            for (int k = 0; k < 13; k++) putLE32(&p[3 + 4 * k], coefs[t * 16 + k]);
            putLE32(&p[55], (uint32_t)nMI);
            putLE32(&p[59], (uint32_t)nMX);
            if (valueChecksum) putLE32(&p[63], coefs[t * 16 + 13]);   // LsHeader.packHeader :259-261
            memcpy(&p[hdrDeflate], zInit.data(), zInit.size());
            memcpy(&p[hdrDeflate + zInit.size()], zInt.data(), zInt.size());
        });
    }
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        offsets[t] = total;
        if (st[t] == GF_OK) total += alt[t].empty() ? lengths[t] : alt[t].size();
        if (types) types[t] = st[t] == GF_OK ? (alt[t].empty() ? 2 : 1) : 0;
    }
    offsets[nTiles] = total;
    if (status) memcpy(status, st.data(), nTiles * 4);
    if (total > blobCap) return GF_ERR_CAPACITY;
    for (size_t t = 0; t < nTiles; t++) {
        if (st[t] != GF_OK) continue;
        if (alt[t].empty()) memcpy(blob + offsets[t], slots.data() + t * stride, lengths[t]);
        else memcpy(blob + offsets[t], alt[t].data(), alt[t].size());
    }
    return GF_OK;
}

// LsDecoder12.decode :94-160 for a batch in host memory.  Every container type is decoded on the GPU as stored: canonical
// Huffman (type 2), legacy Huffman of M32 (type 0, either header revision) and Deflate (type 1: the two zlib streams are
// inflated by k_inflate).  The host only moves bytes.
gf_status gf_lsop12_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                     const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !blob || !offsets || !values) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;    // a bad array must not become an out-of-bounds read
    GF_HIP(hipSetDevice(c->device));
    if (nRows < 6 || nCols < 6) {
        for (size_t t = 0; t < nTiles && status; t++) status[t] = GF_ERR_BOUNDS;
        return GF_OK;
    }
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t nRes = gf_lsop12_residual_count(nRows, nCols), resStride = roundUp(nRes, 4);
    // staging: blob | offsets | lengths | values | statuses | residuals | coefficients | the second status
    std::vector<uint32_t> lengths(nTiles);
    std::vector<int32_t> st(nTiles);
    for (size_t t = 0; t < nTiles; t++) lengths[t] = (uint32_t)(offsets[t + 1] - offsets[t]);
    const size_t total = (size_t)offsets[nTiles];
    HostStage sg(c);
    const int blobP = sg.in(blob, total, 32), offsetsP = sg.in(offsets, (nTiles + 1) * 8), lengthsP = sg.in(lengths.data(), nTiles * 4);
    const int valuesP = sg.out(values, nTiles * cells * 4), statusP = sg.out(st.data(), nTiles * 4);
    const int resP = sg.local(nTiles * resStride * 4), coefsP = sg.local(nTiles * 64), status2P = sg.local(nTiles * 4);
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    s = gf_lsop12_decode_batch_i32_dev(c, c->stream, nRows, nCols, nTiles, sg.ptr<uint8_t>(blobP), total, sg.ptr<uint64_t>(offsetsP), 0,
                                       sg.ptr<uint32_t>(lengthsP), sg.ptr<int32_t>(valuesP), sg.ptr<int32_t>(statusP), sg.ptr<int32_t>(resP),
                                       resStride, sg.ptr<uint32_t>(coefsP), sg.ptr<int32_t>(status2P));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    if (status) memcpy(status, st.data(), nTiles * 4);
    return GF_OK;
}

gf_status gf_lsop12_encode_i32(gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values, int deflateEnabled,
                               uint8_t *out, size_t outCap, size_t *outLen)
{
    GF_CTX_LOCK(c);
    return oneTileEncode(outLen, [&](uint64_t *offsets, int32_t *st) {
        return gf_lsop12_encode_batch_i32(c, codecIndex, nRows, nCols, 1, values, deflateEnabled, out, outCap, offsets, nullptr, st);
    });
}

gf_status gf_lsop12_decode_i32(gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, int32_t *values)
{
    GF_CTX_LOCK(c);
    return oneTileDecode(len, [&](const uint64_t *offsets, int32_t *st) {
        return gf_lsop12_decode_batch_i32(c, nRows, nCols, 1, packing, offsets, values, st);
    });
}

// ------------------------------------------------------------------ LSOP08

// the shapes the LSOP08 kernels take: LsOptimalPredictor08.java:62-64 declines fewer than 4 rows or columns (the callers answer
// that themselves); k_lsop8_reconstruct keeps two rows of a tile in LDS; the packer counts a packing's bits in 32 bits
static gf_status lsop08Shape(int nRows, int nCols)
{
    if (nCols > GF_LSOP8_MAX_COLS || (size_t)nRows * (size_t)nCols >= (1ull << 26)) return GF_ERR_UNSUPPORTED;
    return GF_OK;
}

size_t gf_lsop08_residual_count(int nRows, int nCols)
{
    if (nRows < 4 || nCols < 4) return 0;
    return (size_t)2 * nRows + (size_t)2 * nCols - 5 + (size_t)(nRows - 2) * (size_t)(nCols - 2);
}

size_t gf_lsop08_max_packing(int nRows, int nCols)
{
    // 47 header bytes + two bodies.  Huffman: a serialised tree is at most 8 + 10 * 256 - 1 bits and the text no longer than the M32
    // bytes themselves (a Huffman code of at most 256 symbols is never longer than the fixed 8-bit one); Deflate: the reference
    // gives each zlib stream its input's length + 128.  A value has at most 6 M32 bytes.
    const size_t n = gf_lsop08_residual_count(nRows, nCols);
    if (n == 0) return 0;
    return roundUp(47 + 2 * 328 + 6 * n + 16, 16);
}

gf_status gf_lsop08_predict_dev(gf_context *c, int nRows, int nCols, size_t nTiles, const int32_t *dValues, int32_t *dResiduals,
                                size_t resStride, uint32_t *dCoefs, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dResiduals || !dCoefs || !dStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (nRows < 4 || nCols < 4) {                       // LsOptimalPredictor08.java:62-64 -> null
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, c->stream));
        return GF_OK;
    }
    if (resStride < gf_lsop08_residual_count(nRows, nCols)) return GF_ERR_ARG;
    const gf_status s = lsop08Shape(nRows, nCols);
    if (s != GF_OK) return s;
    GF_HIP(gf_launch_lsop8_predict(dValues, dResiduals, resStride, dCoefs, dStatus, nTiles, nRows, nCols, c->stream));
    return GF_OK;
}

gf_status gf_lsop08_reconstruct_dev(gf_context *c, int nRows, int nCols, size_t nTiles, const int32_t *dResiduals, size_t resStride,
                                    const uint32_t *dCoefs, const int32_t *dInStatus, int32_t *dValues, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dResiduals || !dCoefs || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (nRows < 4 || nCols < 4 || resStride < gf_lsop08_residual_count(nRows, nCols)) return GF_ERR_ARG;
    const gf_status s = lsop08Shape(nRows, nCols);
    if (s != GF_OK) return s;
    GF_HIP(gf_launch_lsop8_reconstruct(dResiduals, resStride, dCoefs, dInStatus, dValues, dStatus, nTiles, nRows, nCols, c->stream));
    return GF_OK;
}

gf_status gf_lsop08_encode_batch_i32_dev(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *dValues,
                                         uint8_t *dOut, size_t slotStride, uint32_t *dLengths, int32_t *dStatus, int32_t *dResiduals,
                                         size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dOut || !dLengths || !dStatus || !dResiduals || !dCoefs || !dScratchStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (slotStride % 16 != 0 || ((uintptr_t)dOut & 15) != 0 || slotStride < 64) return GF_ERR_ARG;
    if (nRows < 4 || nCols < 4) {
        if (nTiles) {
            GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, c->stream));
            GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dLengths, 0, nTiles, c->stream));
        }
        return GF_OK;
    }
    const gf_status s = gf_lsop08_predict_dev(c, nRows, nCols, nTiles, dValues, dResiduals, resStride, dCoefs, dScratchStatus);
    if (s != GF_OK) return s;
    GF_HIP(gf_launch_lsop8_pack(dResiduals, resStride, dCoefs, dScratchStatus, dOut, slotStride, dLengths, dStatus, nTiles, nRows, nCols,
                                codecIndex, c->stream));
    return GF_OK;
}

gf_status gf_lsop08_decode_batch_i32_dev(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                                         const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues,
                                         int32_t *dStatus, int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dBlob || !dLengths || !dValues || !dStatus || !dResiduals || !dCoefs || !dScratchStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (((uintptr_t)dBlob & 3) != 0) return GF_ERR_ARG;
    const hipStream_t st = c->stream;
    if (nRows < 4 || nCols < 4) {
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_ERR_BOUNDS, nTiles, st));
        return GF_OK;
    }
    if (resStride < gf_lsop08_residual_count(nRows, nCols)) return GF_ERR_ARG;
    gf_status s = lsop08Shape(nRows, nCols);
    if (s != GF_OK || nTiles == 0) return s;
    // every container is k_lsop_unpack_m32's (there is no canonical type): all tiles start out marked for it, the record's spare
    // words as zero
    GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dScratchStatus, GF_ERR_UNSUPPORTED, nTiles, st));
    GF_HIP(hipMemsetAsync(dCoefs, 0, nTiles * 64, st));
    s = lsopUnpackM32Deflate(c, st, gf_lsop08_form(nRows, nCols), nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths,
                             dResiduals, resStride, dCoefs, dScratchStatus);
    if (s != GF_OK) return s;
    GF_HIP(gf_launch_lsop8_reconstruct(dResiduals, resStride, dCoefs, dScratchStatus, dValues, dStatus, nTiles, nRows, nCols, st));
    return GF_OK;
}

// LsEncoder08.encode :66-137 for a batch in host memory: the Huffman body (type 0) comes from the GPU, the host's zlib (level 6)
// compresses the two M32 streams, and the Huffman body is kept only where it is STRICTLY shorter (:118); otherwise the packing is the
// Deflate one (type 1).  types[t] (may be null) = container type written.  A tile whose zlib stream would need more than its input's
// length + 128 bytes -- the reference's buffer, which it would silently cut (:90-101) -- is GF_ERR_UNSUPPORTED.
gf_status gf_lsop08_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values, uint8_t *blob,
                                     size_t blobCap, uint64_t *offsets, uint8_t *types, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (nRows < 4 || nCols < 4) {
        for (size_t t = 0; t <= nTiles; t++) offsets[t] = 0;
        for (size_t t = 0; t < nTiles; t++) { if (status) status[t] = GF_DECLINED; if (types) types[t] = 0; }
        return GF_OK;
    }
    gf_status s = lsop08Shape(nRows, nCols);
    if (s != GF_OK) return s;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t nRes = gf_lsop08_residual_count(nRows, nCols), resStride = roundUp(nRes, 4);
    const GfLsopForm form = gf_lsop08_form(nRows, nCols);
    const size_t nInit = form.nInit, nInt = form.nInt, stride = gf_lsop08_max_packing(nRows, nCols), hdr = 47;
    // staging: values | slots | lengths | statuses | residuals | coefficients | the second status
    std::vector<uint32_t> lengths(nTiles), coefs(nTiles * 16);
    std::vector<int32_t> st(nTiles), res(nTiles * resStride);
    std::vector<uint8_t> slots(nTiles * stride);
    HostStage sg(c);
    const int valuesP = sg.in(values, nTiles * cells * 4), slotsP = sg.out(slots.data(), nTiles * stride);
    const int lengthsP = sg.out(lengths.data(), nTiles * 4), statusP = sg.out(st.data(), nTiles * 4);
    const int resP = sg.out(res.data(), nTiles * resStride * 4), coefsP = sg.out(coefs.data(), nTiles * 64), status2P = sg.local(nTiles * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    s = gf_lsop08_encode_batch_i32_dev(c, codecIndex, nRows, nCols, nTiles, sg.ptr<int32_t>(valuesP), sg.ptr<uint8_t>(slotsP), stride,
                                       sg.ptr<uint32_t>(lengthsP), sg.ptr<int32_t>(statusP), sg.ptr<int32_t>(resP), resStride,
                                       sg.ptr<uint32_t>(coefsP), sg.ptr<int32_t>(status2P));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;

    std::vector<std::vector<uint8_t>> alt(nTiles);          // the Deflate container where the Huffman body is not strictly shorter
    parallelFor(nTiles, [&](size_t t) {
        if (st[t] != GF_OK) return;
        const int32_t *r = res.data() + t * resStride;
        std::vector<uint8_t> mInit, mInt, zInit, zInt;
        const size_t nMI = m32Pack(r, nInit, mInit), nMX = m32Pack(r + nInit, nInt, mInt);
        if (!zDeflate(mInit.data(), nMI, 6, zInit) || !zDeflate(mInt.data(), nMX, 6, zInt) || zInit.size() > nMI + 128 ||
            zInt.size() > nMX + 128) {
            st[t] = GF_ERR_UNSUPPORTED;
            return;
        }
        if (lengths[t] - hdr < zInit.size() + zInt.size()) return;                  // :118
        std::vector<uint8_t> &p = alt[t];
        p.resize(hdr + zInit.size() + zInt.size());
        p[0] = (uint8_t)codecIndex;
        p[1] = 0x41;                                         // COMPRESSION_TYPE_DEFLATE | REVISION_FLAG
        p[2] = 8;
        for (int k = 0; k < 9; k++) putLE32(&p[3 + 4 * k], coefs[t * 16 + k]);
        putLE32(&p[39], (uint32_t)nMI);
        putLE32(&p[43], (uint32_t)nMX);
        memcpy(&p[hdr], zInit.data(), zInit.size());
        memcpy(&p[hdr + zInit.size()], zInt.data(), zInt.size());
    });
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        offsets[t] = total;
        if (st[t] == GF_OK) total += alt[t].empty() ? lengths[t] : alt[t].size();
        if (types) types[t] = st[t] == GF_OK && !alt[t].empty() ? 1 : 0;
    }
    offsets[nTiles] = total;
    if (status) memcpy(status, st.data(), nTiles * 4);
    if (total > blobCap) return GF_ERR_CAPACITY;
    for (size_t t = 0; t < nTiles; t++) {
        if (st[t] != GF_OK) continue;
        if (alt[t].empty()) memcpy(blob + offsets[t], slots.data() + t * stride, lengths[t]);
        else memcpy(blob + offsets[t], alt[t].data(), alt[t].size());
    }
    return GF_OK;
}

// LsDecoder08.decode :71-116 for a batch in host memory: both container types and both header revisions, decoded on the GPU as stored
gf_status gf_lsop08_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                                     int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !blob || !offsets || !values) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (nRows < 4 || nCols < 4) {
        for (size_t t = 0; t < nTiles && status; t++) status[t] = GF_ERR_BOUNDS;
        return GF_OK;
    }
    gf_status s = lsop08Shape(nRows, nCols);
    if (s != GF_OK) return s;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t nRes = gf_lsop08_residual_count(nRows, nCols), resStride = roundUp(nRes, 4);
    // staging: blob | offsets | lengths | values | statuses | residuals | coefficients | the second status
    std::vector<uint32_t> lengths(nTiles);
    std::vector<int32_t> st(nTiles);
    for (size_t t = 0; t < nTiles; t++) lengths[t] = (uint32_t)(offsets[t + 1] - offsets[t]);
    const size_t total = (size_t)offsets[nTiles];
    HostStage sg(c);
    const int blobP = sg.in(blob, total, 32), offsetsP = sg.in(offsets, (nTiles + 1) * 8), lengthsP = sg.in(lengths.data(), nTiles * 4);
    const int valuesP = sg.out(values, nTiles * cells * 4), statusP = sg.out(st.data(), nTiles * 4);
    const int resP = sg.local(nTiles * resStride * 4), coefsP = sg.local(nTiles * 64), status2P = sg.local(nTiles * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    s = gf_lsop08_decode_batch_i32_dev(c, nRows, nCols, nTiles, sg.ptr<uint8_t>(blobP), total, sg.ptr<uint64_t>(offsetsP), 0,
                                       sg.ptr<uint32_t>(lengthsP), sg.ptr<int32_t>(valuesP), sg.ptr<int32_t>(statusP), sg.ptr<int32_t>(resP),
                                       resStride, sg.ptr<uint32_t>(coefsP), sg.ptr<int32_t>(status2P));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    if (status) memcpy(status, st.data(), nTiles * 4);
    return GF_OK;
}

gf_status gf_lsop08_encode_i32(gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values, uint8_t *out, size_t outCap,
                               size_t *outLen)
{
    GF_CTX_LOCK(c);
    return oneTileEncode(outLen, [&](uint64_t *offsets, int32_t *st) {
        return gf_lsop08_encode_batch_i32(c, codecIndex, nRows, nCols, 1, values, out, outCap, offsets, nullptr, st);
    });
}

gf_status gf_lsop08_decode_i32(gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, int32_t *values)
{
    GF_CTX_LOCK(c);
    return oneTileDecode(len, [&](const uint64_t *offsets, int32_t *st) {
        return gf_lsop08_decode_batch_i32(c, nRows, nCols, 1, packing, offsets, values, st);
    });
}

}  // extern "C"
