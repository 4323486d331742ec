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
    const size_t rawStride = roundUp(6 * (nInit + nInt) + 192, 16);       // (a value has at most 6 M32 bytes)
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

static_assert(GF_LSOP08.maxCols == GF_LSOP8_MAX_COLS, "the family table states the LSOP08 kernels' column limit");

// (round 6, advice) int32Residuals: the caller reads d_residuals itself (the host form's Deflate stage) -- a parameter of
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
    if (GF_LSOP12.tooSmall(nRows, nCols)) {
        if (nTiles) {
            GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, st));
            GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dLengths, 0, nTiles, st));
        }
        return GF_OK;
    }
    // Terrain-sized tiles (round 5): the first kernel keeps the tile in LDS as halfwords, writes the residuals as int16 and counts
    // the histograms on the way (k_lsop_predict16; records in the context's selection-record buffer, which gf_context_reserve
    // sizes) -- unless the caller wants the int32 residuals themselves (int32Residuals: the host's Deflate stage)
    const bool fast16 = gf_lsop_predict16_eligible(nRows, nCols) && !int32Residuals && resStride >= GF_LSOP12.residualCount(nRows, nCols);
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
    const GfLsopForm form = gf_lsop12_form(nRows, nCols);
    const uint32_t n0 = form.nInit, n1 = form.nInt;
    if (4ull * ((uint64_t)n1 + 1) >= (1ull << 22)) return GF_ERR_UNSUPPORTED;       // 22-bit counts in the tree keys
    const int valueChecksum = (flags & GF_LSOP_VALUE_CHECKSUM) ? 1 : 0;
    if (valueChecksum)
        GF_HIP(gf_launch_lsop_value_crc(dValues, (size_t)nRows * (size_t)nCols, nTiles, nullptr, dCoefs, st));
    GF_HIP(gf_launch_canon_pack2(dResiduals, resStride, dCoefs, dScratchStatus, dOut, slotStride, dLengths, dStatus, nTiles,
                                 n0, n1, codecIndex, st, valueChecksum, hist16));
    return GF_OK;
}

// The encoder of a family for a batch in host memory (LsEncoder12.encode :122-219, LsEncoder08.encode :66-137): the device's packing
// comes from devEncode (the family's _dev form on the staged arrays); with deflate the host's zlib compresses the two M32 streams and
// the family's rule chooses (gvrs_lsop_container.h).  Residuals and coefficient records come home for that alone: without deflate
// (LSOP12's switch; LSOP08 has none) they stay on the device.
template <class DevEncode>
static gf_status lsopEncodeBatchHost(const LsopFamily &F, gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                     bool deflate, bool valueChecksum, uint8_t *blob, size_t blobCap, uint64_t *offsets,
                                     uint8_t *types, int32_t *status, DevEncode devEncode)
{
    if (!c || nRows < 1 || nCols < 1 || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (F.tooSmall(nRows, nCols)) {
        for (size_t t = 0; t <= nTiles; t++) offsets[t] = 0;
        for (size_t t = 0; t < nTiles; t++) { if (status) status[t] = GF_DECLINED; if (types) types[t] = 0; }
        return GF_OK;
    }
    if (F.hostFormsCheckShape && F.tooLarge(nRows, nCols)) return GF_ERR_UNSUPPORTED;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t resStride = roundUp(F.residualCount(nRows, nCols), 4), stride = F.maxPacking(nRows, nCols);
    // staging: values | slots | lengths | statuses | residuals | coefficients | the second status
    std::vector<uint32_t> lengths(nTiles), coefs(deflate ? nTiles * 16 : 0);
    std::vector<int32_t> st(nTiles), res(deflate ? nTiles * resStride : 0);
    std::vector<uint8_t> slots(nTiles * stride);
    HostStage sg(c);
    const int valuesP = sg.in(values, nTiles * cells * 4), slotsP = sg.out(slots.data(), nTiles * stride);
    const int lengthsP = sg.out(lengths.data(), nTiles * 4), statusP = sg.out(st.data(), nTiles * 4);
    const int resP = deflate ? sg.out(res.data(), nTiles * resStride * 4) : sg.local(nTiles * resStride * 4);
    const int coefsP = deflate ? sg.out(coefs.data(), nTiles * 64) : sg.local(nTiles * 64);
    const int status2P = sg.local(nTiles * 4);
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    s = devEncode(sg.ptr<int32_t>(valuesP), sg.ptr<uint8_t>(slotsP), stride, sg.ptr<uint32_t>(lengthsP), sg.ptr<int32_t>(statusP),
                  sg.ptr<int32_t>(resP), resStride, sg.ptr<uint32_t>(coefsP), sg.ptr<int32_t>(status2P));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    std::vector<std::vector<uint8_t>> alt;                  // the Deflate container where it wins
    lsopAlternatives(F, codecIndex, deflate, valueChecksum, nRows, nCols, nTiles, res.data(), resStride, coefs.data(), lengths.data(), st.data(),
                     alt, [](size_t n, auto f) { parallelFor(n, f); });
    return lsopAssemble(F, nTiles, st.data(), lengths.data(), slots.data(), stride, alt, blob, blobCap, offsets, types, status);
}

// The decoder of a family for a batch in host memory (LsDecoder12.decode :94-160, LsDecoder08.decode :71-116): every container type
// and either header revision is decoded on the GPU as stored by devDecode (the family's _dev form on the staged arrays; Deflate
// containers: the two zlib streams are inflated by k_inflate).  The host only moves bytes.
template <class DevDecode>
static gf_status lsopDecodeBatchHost(const LsopFamily &F, gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                     const uint64_t *offsets, int32_t *values, int32_t *status, DevDecode devDecode)
{
    if (!c || nRows < 1 || nCols < 1 || !blob || !offsets || !values) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;    // a bad array must not become an out-of-bounds read
    GF_HIP(hipSetDevice(c->device));
    if (F.tooSmall(nRows, nCols)) {
        for (size_t t = 0; t < nTiles && status; t++) status[t] = GF_ERR_BOUNDS;
        return GF_OK;
    }
    if (F.hostFormsCheckShape && F.tooLarge(nRows, nCols)) return GF_ERR_UNSUPPORTED;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t resStride = roundUp(F.residualCount(nRows, nCols), 4);
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
    s = devDecode(sg.ptr<uint8_t>(blobP), total, sg.ptr<uint64_t>(offsetsP), sg.ptr<uint32_t>(lengthsP), sg.ptr<int32_t>(valuesP),
                  sg.ptr<int32_t>(statusP), sg.ptr<int32_t>(resP), resStride, sg.ptr<uint32_t>(coefsP), sg.ptr<int32_t>(status2P));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    if (status) memcpy(status, st.data(), nTiles * 4);
    return GF_OK;
}

extern "C" {

// ------------------------------------------------------------------ LSOP12

size_t gf_lsop12_residual_count(int nRows, int nCols) { return GF_LSOP12.residualCount(nRows, nCols); }

size_t gf_lsop12_max_packing(int nRows, int nCols) { return GF_LSOP12.maxPacking(nRows, nCols); }

gf_status gf_lsop12_predict_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const int32_t *dValues,
                                int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dResiduals || !dCoefs || !dStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    if (GF_LSOP12.tooLarge(nRows, nCols)) return GF_ERR_UNSUPPORTED;
    const hipStream_t st = streamOf(c, stream);
    if (GF_LSOP12.tooSmall(nRows, nCols)) {             // LsOptimalPredictor12.java:114-116 -> null
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, st));
        return GF_OK;
    }
    if (resStride < GF_LSOP12.residualCount(nRows, nCols)) return GF_ERR_ARG;
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
    if (GF_LSOP12.tooSmall(nRows, nCols) || resStride < GF_LSOP12.residualCount(nRows, nCols)) return GF_ERR_ARG;
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
    if (GF_LSOP12.tooSmall(nRows, nCols)) {
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_ERR_BOUNDS, nTiles, st));
        return GF_OK;
    }
    if (resStride < GF_LSOP12.residualCount(nRows, nCols)) return GF_ERR_ARG;
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

// LsEncoder12.encode for a batch in host memory.  deflateEnabled carries LsEncoder12's two switches as bits: GF_LSOP_DEFLATE
// (setDeflateEnabled, default true: the Deflate container replaces the GPU's canonical-Huffman packing when strictly smaller) and
// GF_LSOP_VALUE_CHECKSUM (setValueChecksumEnabled); any other bit is refused.  types[t] = container type written (2 / 1).
gf_status gf_lsop12_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                     int deflateEnabled, uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *types,
                                     int32_t *status)
{
    GF_CTX_LOCK(c);
    if (deflateEnabled & ~(GF_LSOP_DEFLATE | GF_LSOP_VALUE_CHECKSUM)) return GF_ERR_ARG;      // (a bit mask since round 5: see the header)
    const bool deflate = (deflateEnabled & GF_LSOP_DEFLATE) != 0, valueChecksum = (deflateEnabled & GF_LSOP_VALUE_CHECKSUM) != 0;
    return lsopEncodeBatchHost(GF_LSOP12, c, codecIndex, nRows, nCols, nTiles, values, deflate, valueChecksum, blob, blobCap, offsets,
                               types, status, [&](const int32_t *dValues, uint8_t *dOut, size_t slotStride, uint32_t *dLengths, int32_t *dStatus,
                                                  int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus) {
        return lsopEncodeBatchDev(c, c->stream, codecIndex, nRows, nCols, nTiles, dValues, valueChecksum ? GF_LSOP_VALUE_CHECKSUM : 0, deflate,
                                  dOut, slotStride, dLengths, dStatus, dResiduals, resStride, dCoefs, dScratchStatus);
    });
}

gf_status gf_lsop12_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                     const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    return lsopDecodeBatchHost(GF_LSOP12, c, nRows, nCols, nTiles, blob, offsets, values, status,
                               [&](const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets, const uint32_t *dLengths, int32_t *dValues,
                                   int32_t *dStatus, int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus) {
        return gf_lsop12_decode_batch_i32_dev(c, c->stream, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, 0, dLengths, dValues, dStatus,
                                              dResiduals, resStride, dCoefs, dScratchStatus);
    });
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

// the shapes the LSOP08 kernels take (fewer than 4 rows or columns: the callers answer that themselves)
static gf_status lsop08Shape(int nRows, int nCols) { return GF_LSOP08.tooLarge(nRows, nCols) ? GF_ERR_UNSUPPORTED : GF_OK; }

size_t gf_lsop08_residual_count(int nRows, int nCols) { return GF_LSOP08.residualCount(nRows, nCols); }

size_t gf_lsop08_max_packing(int nRows, int nCols) { return GF_LSOP08.maxPacking(nRows, nCols); }

gf_status gf_lsop08_predict_dev(gf_context *c, int nRows, int nCols, size_t nTiles, const int32_t *dValues, int32_t *dResiduals,
                                size_t resStride, uint32_t *dCoefs, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dValues || !dResiduals || !dCoefs || !dStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (GF_LSOP08.tooSmall(nRows, nCols)) {             // LsOptimalPredictor08.java:62-64 -> null
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_DECLINED, nTiles, c->stream));
        return GF_OK;
    }
    if (resStride < GF_LSOP08.residualCount(nRows, nCols)) return GF_ERR_ARG;
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
    if (GF_LSOP08.tooSmall(nRows, nCols) || resStride < GF_LSOP08.residualCount(nRows, nCols)) return GF_ERR_ARG;
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
    if (GF_LSOP08.tooSmall(nRows, nCols)) {
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
    return lsop08DecodeDev(c, c ? c->stream : nullptr, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride, dLengths, dValues, dStatus,
                           dResiduals, resStride, dCoefs, dScratchStatus);
}

}  // extern "C"

// ... on a stream: the records' driver runs a list's LSOP08 entry on its caller's (gvrs_api_records_dev.hip)
gf_status lsop08DecodeDev(gf_context *c, hipStream_t st, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                          const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus,
                          int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus)
{
    GF_CTX_LOCK(c);
    if (!c || !dBlob || !dLengths || !dValues || !dStatus || !dResiduals || !dCoefs || !dScratchStatus || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    if (((uintptr_t)dBlob & 3) != 0) return GF_ERR_ARG;
    if (GF_LSOP08.tooSmall(nRows, nCols)) {
        if (nTiles) GF_HIP(hipMemsetD32Async((hipDeviceptr_t)dStatus, GF_ERR_BOUNDS, nTiles, st));
        return GF_OK;
    }
    if (resStride < GF_LSOP08.residualCount(nRows, nCols)) return GF_ERR_ARG;
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

extern "C" {

// LsEncoder08.encode for a batch in host memory: the Huffman container (type 0) comes from the GPU and is kept only where its body is
// STRICTLY shorter than the two zlib streams (:118); otherwise the packing is the Deflate one (type 1).  types[t] (may be null) =
// container type written.  A tile whose zlib stream would need more than its input's length + 128 bytes is GF_ERR_UNSUPPORTED.
gf_status gf_lsop08_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values, uint8_t *blob,
                                     size_t blobCap, uint64_t *offsets, uint8_t *types, int32_t *status)
{
    GF_CTX_LOCK(c);
    return lsopEncodeBatchHost(GF_LSOP08, c, codecIndex, nRows, nCols, nTiles, values, true, false, blob, blobCap, offsets, types, status,
                               [&](const int32_t *dValues, uint8_t *dOut, size_t slotStride, uint32_t *dLengths, int32_t *dStatus,
                                   int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus) {
        return gf_lsop08_encode_batch_i32_dev(c, codecIndex, nRows, nCols, nTiles, dValues, dOut, slotStride, dLengths, dStatus, dResiduals,
                                              resStride, dCoefs, dScratchStatus);
    });
}

gf_status gf_lsop08_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                                     int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    return lsopDecodeBatchHost(GF_LSOP08, c, nRows, nCols, nTiles, blob, offsets, values, status,
                               [&](const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets, const uint32_t *dLengths, int32_t *dValues,
                                   int32_t *dStatus, int32_t *dResiduals, size_t resStride, uint32_t *dCoefs, int32_t *dScratchStatus) {
        return gf_lsop08_decode_batch_i32_dev(c, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, 0, dLengths, dValues, dStatus, dResiduals,
                                              resStride, dCoefs, dScratchStatus);
    });
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
