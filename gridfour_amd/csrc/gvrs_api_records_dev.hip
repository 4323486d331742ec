// gvrs_api_records_dev.hip -- tile records and mixed-codec packings decoded where they lie in device memory: what
// gf_tile_record_decode_batch and gf_codec_master_decode_batch_i32 do on the host (walk the framing, verify the CRC-32C, sort the
// packings by codec, narrow shorts, copy raw tiles) as four kernels of gvrs_records.hip around the codecs' device decoders.
// ONE driver (recordsDecodeDev) serves gf_tile_record_decode_batch_elems_dev, the one-element gf_tile_record_decode_batch_dev,
// gf_codec_master_decode_batch_i32_dev (packings without framing) and the host-staged gf_tile_record_decode_batch_elems: every
// element of every record is one INSTANCE, the instances lie element-major (i = e * nTiles + t), and one partition by codec index,
// one count read-back and one launch per codec serve all elements together.
// Reference: gvrs/RecordManager.java:492-515, gvrs/RasterTile.java:234-256, TileElement{Int,Short,Float,IntCodedFloat}.decode,
// gvrs/CodecMaster.java:195-203 (decode), 296-304 (decodeFloats).

#include "gvrs_api_internal.h"

namespace {

// one codec's share of the batch through its device decoder: packing j = lengths[j] bytes at dBlob + offsets[j]; the entry that is
// GF_CODEC_NONE is the slot of CodecFloat, whose cells are float bit patterns
gf_status decodeSublist(gf_context *c, hipStream_t st, int codec, int nRows, int nCols, size_t n, const uint8_t *dBlob, size_t blobBytes,
                        const uint64_t *offsets, const uint32_t *lengths, int32_t *values, int32_t *status)
{
    switch (codec) {
    case GF_CODEC_NONE: return floatDecodeDev(c, st, nRows, nCols, n, dBlob, blobBytes, offsets, lengths, (float *)values, status);
    case GF_CODEC_HUFFMAN: return decodeBatchDev(KIND_HUFFMAN, c, st, nRows, nCols, n, dBlob, blobBytes, offsets, 0, lengths, values, status, 0);
    case GF_CODEC_CANON_HUFFMAN: return decodeBatchDev(KIND_CANON, c, st, nRows, nCols, n, dBlob, blobBytes, offsets, 0, lengths, values, status, 0);
    case GF_CODEC_DEFLATE: return deflateDecodeDev(c, st, nRows, nCols, n, dBlob, blobBytes, offsets, 0, lengths, values, status);
    case GF_CODEC_LSOP12: {
        const size_t resStride = roundUp(gf_lsop12_residual_count(nRows, nCols), 4);
        gf_status s;
        if ((s = c->dResiduals.ensure(n * resStride * 4 + 16)) != GF_OK) return s;
        if ((s = c->dCoefs.ensure(n * 64 + 16)) != GF_OK) return s;
        if ((s = c->dStatus2.ensure(n * 4 + 16)) != GF_OK) return s;
        return gf_lsop12_decode_batch_i32_dev(c, st, nRows, nCols, n, dBlob, blobBytes, offsets, 0, lengths, values, status,
                                              (int32_t *)c->dResiduals.p, resStride, (uint32_t *)c->dCoefs.p, (int32_t *)c->dStatus2.p);
    }
    case GF_CODEC_LSOP08: {
        const size_t resStride = roundUp(GF_LSOP08.residualCount(nRows, nCols), 4);
        gf_status s;
        if ((s = c->dResiduals.ensure(n * resStride * 4 + 16)) != GF_OK) return s;
        if ((s = c->dCoefs.ensure(n * 64 + 16)) != GF_OK) return s;
        if ((s = c->dStatus2.ensure(n * 4 + 16)) != GF_OK) return s;
        return lsop08DecodeDev(c, st, nRows, nCols, n, dBlob, blobBytes, offsets, 0, lengths, values, status, (int32_t *)c->dResiduals.p,
                               resStride, (uint32_t *)c->dCoefs.p, (int32_t *)c->dStatus2.p);
    }
    default: return GF_ERR_ARG;
    }
}

}  // namespace

// what the host can check without a device (values: device or host pointers, only looked at for null); a negative nCodecs is an
// empty list
gf_status elemsArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                    size_t nTiles, const uint8_t *blob, bool blobOnDevice, const uint64_t *offsets, void *const *values,
                    const int32_t *status)
{
    if (!c || !elems || !blob || !offsets || !values || !status || (!codecs && nCodecs > 0)) return GF_ERR_ARG;
    if (nElems < 1 || nElems > GF_MAX_ELEMS || nRows < 1 || nCols < 1 || nCodecs > 255) return GF_ERR_ARG;
    if (blobOnDevice && ((uintptr_t)blob & 3) != 0) return GF_ERR_ARG;
    for (int e = 0; e < nElems; e++) {
        if (!values[e] || elems[e].type < GF_ELEM_INT || elems[e].type > GF_ELEM_ICF) return GF_ERR_ARG;
        if (elems[e].type == GF_ELEM_ICF && (elems[e].scale == 0.0f || std::isnan(elems[e].scale))) return GF_ERR_ARG;
    }
    for (int k = 0; k < nCodecs; k++)
        if (codecs[k] < GF_CODEC_NONE || codecs[k] > GF_CODEC_LSOP08) return GF_ERR_ARG;
    if (nTiles > 0x7fffffffull / (size_t)nElems) return GF_ERR_UNSUPPORTED;         // instance numbers travel as 32 bits
    return GF_OK;
}

size_t elemItemBytes(int type) { return type == GF_ELEM_SHORT ? 2 : 4; }

// the one device pipeline.  dLengths == nullptr: tile records, record t = [dOffsets[t], dOffsets[t + 1]), or [dOffsets[t], dEnds[t])
// where dEnds is given (records anywhere in a file image: gvrs_api_file.hip).  Else packing mode: one INT element, packing t =
// dLengths[t] bytes at dOffsets[t], no framing, no standard form, no checksum, no tile index.
gf_status recordsDecodeDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows,
                           int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                           const uint32_t *dLengths, int verifyChecksum, int32_t *dTileIndices, void *const *dValues, int32_t *dStatus,
                           const uint64_t *dEnds)
{
    if (nCodecs < 0) nCodecs = 0;
    const size_t cells = (size_t)nRows * (size_t)nCols, n = nTiles, nInst = (size_t)nElems * n;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = streamOf(c, stream);
    const int nSeg = nCodecs + 1;                                                 // the codecs, then the standard form
    // per instance (a multiple of 4 of them): start, length, class; per record: size.  The partition: per instance offset, length,
    // destination, status; the segments' counts; the element table
    const size_t nPad = roundUp(nInst, 4);
    Carve meta, sub;
    const size_t startsAt = meta.add(nPad * 8), lensAt = meta.add(nPad * 4), clsAt = meta.add(nPad * 4), sizesAt = meta.add(n * 4);
    const size_t subOffAt = sub.add(nPad * 8), subLenAt = sub.add(nPad * 4), subDstAt = sub.add(nPad * 4), subStatusAt = sub.add(nPad * 4);
    const size_t countsAt = sub.add(256 * 4), elemsAt = sub.add(GF_MAX_ELEMS * sizeof(GfElemDesc));
    gf_status s;
    if ((s = c->dRecMeta.ensure(meta)) != GF_OK) return s;
    if ((s = c->dRecSub.ensure(sub)) != GF_OK) return s;
    if ((s = c->hRecCounts.ensure(256 * 4)) != GF_OK) return s;
    const DevBuf &M = c->dRecMeta, &S = c->dRecSub;
    uint64_t *starts = M.at<uint64_t>(startsAt), *subOffsets = S.at<uint64_t>(subOffAt);
    uint32_t *lens = M.at<uint32_t>(lensAt), *sizes = M.at<uint32_t>(sizesAt), *subLengths = S.at<uint32_t>(subLenAt), *subDst = S.at<uint32_t>(subDstAt);
    int32_t *cls = M.at<int32_t>(clsAt), *subStatus = S.at<int32_t>(subStatusAt);
    uint32_t *dCounts = S.at<uint32_t>(countsAt);
    GfElemDesc *dElems = S.at<GfElemDesc>(elemsAt);

    // the element table for k_elem_scatter; the walk takes the types as a packed word.  (A pageable source: the runtime has
    // staged the copy when the call returns, and the table outlives the synchronisation below anyway.)
    GfElemDesc table[GF_MAX_ELEMS] = {};
    uint32_t types = 0;
    for (int e = 0; e < nElems; e++) {
        table[e].values = dValues[e];
        table[e].type = elems[e].type;
        table[e].fillI = elems[e].fill_i;
        table[e].scale = elems[e].scale;
        table[e].offset = elems[e].offset;
        table[e].fillF = elems[e].fill_f;
        types |= (uint32_t)elems[e].type << (2 * e);
    }
    GF_HIP(hipMemcpyAsync(dElems, table, (size_t)nElems * sizeof(GfElemDesc), hipMemcpyHostToDevice, st));

    GfRecordParseElemsArgs p{};
    p.blob = dBlob;
    p.blobBytes = blobBytes;
    p.offsets = dOffsets;
    p.ends = dLengths ? nullptr : dEnds;
    p.lengths = dLengths;
    p.nTiles = n;
    p.nElems = nElems;
    p.elemTypes = types;
    p.cells = (uint32_t)cells;
    p.nCodecs = nCodecs;
    uint64_t iset[4] = {0, 0, 0, 0}, fset[4] = {0, 0, 0, 0};
    for (int k = 0; k < nCodecs; k++) (codecs[k] != GF_CODEC_NONE ? iset : fset)[k >> 6] |= 1ull << (k & 63);
    p.intSet0 = iset[0], p.intSet1 = iset[1], p.intSet2 = iset[2], p.intSet3 = iset[3];
    p.floatSet0 = fset[0], p.floatSet1 = fset[1], p.floatSet2 = fset[2], p.floatSet3 = fset[3];
    p.tileIndices = dTileIndices;
    p.starts = starts;
    p.lens = lens;
    p.cls = cls;
    p.status = dStatus;
    p.sizes = sizes;
    GF_HIP(gf_launch_record_parse_elems(p, st));
    if (verifyChecksum && !dLengths) GF_HIP(gf_launch_record_crc32c_elems(dBlob, dOffsets, sizes, cls, dStatus, n, nElems, st));
    GfPartitionArgs q{};
    q.cls = cls;
    q.starts = starts;
    q.lens = lens;
    q.nTiles = nInst;
    q.nCodecs = nCodecs;
    q.subOffsets = subOffsets;
    q.subLengths = subLengths;
    q.subDst = subDst;
    q.counts = dCounts;
    GF_HIP(gf_launch_codec_partition(q, st));
    // the one synchronisation of the call: the host has to know which decoders to launch, and for how many instances
    const uint32_t *counts = (const uint32_t *)c->hRecCounts.p;
    GF_HIP(hipMemcpyAsync(c->hRecCounts.p, dCounts, (size_t)nSeg * 4, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    size_t nPacked = 0;
    for (int k = 0; k < nCodecs; k++) nPacked += counts[k];
    const size_t nStd = counts[nCodecs];
    // one INT or FLOAT element and every record names the same codec: the partition is the identity, the decoder writes to the caller's arrays
    if (nElems == 1 && (elems[0].type == GF_ELEM_INT || elems[0].type == GF_ELEM_FLOAT))
        for (int k = 0; k < nCodecs; k++)
            if (counts[k] == n) return decodeSublist(c, st, codecs[k], nRows, nCols, n, dBlob, blobBytes, starts, lens, (int32_t *)dValues[0], dStatus);
    if (nPacked && (s = c->dRecTmp.ensure(nPacked * cells * 4 + 64)) != GF_OK) return s;
    int32_t *tmp = (int32_t *)c->dRecTmp.p;
    size_t j0 = 0;
    for (int k = 0; k < nCodecs; k++) {                                            // in list order, on the caller's stream
        const size_t nk = counts[k];
        if (!nk) continue;
        s = decodeSublist(c, st, codecs[k], nRows, nCols, nk, dBlob, blobBytes, subOffsets + j0, subLengths + j0, tmp + j0 * cells, subStatus + j0);
        if (s != GF_OK) return s;
        j0 += nk;
    }
    GfElemScatterArgs g{};
    g.blob = dBlob;
    g.tmp = tmp;
    g.subStatus = subStatus;
    g.subOffsets = subOffsets;
    g.subDst = subDst;
    g.nPacked = nPacked;
    g.nTotal = nPacked + nStd;
    g.nTiles = n;
    g.cells = (uint32_t)cells;
    g.elems = dElems;
    g.status = dStatus;
    GF_HIP(gf_launch_elem_scatter(g, st));
    return GF_OK;
}

namespace {

// the checks and the lock that the three device entry points share
gf_status recordsDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                     size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets, const uint32_t *dLengths,
                     int verifyChecksum, int32_t *dTileIndices, void *const *dValues, int32_t *dStatus)
{
    const gf_status s = elemsArgs(c, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, dBlob, true, dOffsets, dValues, dStatus);
    if (s != GF_OK || nTiles == 0) return s;
    GF_CTX_LOCK(c);
    return recordsDecodeDev(c, stream, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, dLengths,
                            verifyChecksum, dTileIndices, dValues, dStatus);
}

}  // namespace

extern "C" {

gf_status gf_tile_record_decode_batch_elems_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems,
                                                int nElems, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                                                const uint64_t *dOffsets, int verifyChecksum, int32_t *dTileIndices, void *const *dValues,
                                                int32_t *dStatus)
{
    return recordsDev(c, stream, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, nullptr, verifyChecksum,
                      dTileIndices, dValues, dStatus);
}

gf_status gf_tile_record_decode_batch_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, int elemType, int nRows,
                                          int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                                          int verifyChecksum, int32_t *dTileIndices, void *dValues, int32_t *dStatus)
{
    if (elemType != GF_ELEM_INT && elemType != GF_ELEM_SHORT) return GF_ERR_ARG;
    gf_elem_spec elem{};
    elem.type = elemType;
    elem.scale = 1.0f;
    void *const values[1] = {dValues};
    return recordsDev(c, stream, codecs, nCodecs, &elem, 1, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, nullptr, verifyChecksum,
                      dTileIndices, values, dStatus);
}

gf_status gf_codec_master_decode_batch_i32_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, int nRows, int nCols,
                                               size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                                               const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus)
{
    if (!dLengths || !codecs || nCodecs < 1) return GF_ERR_ARG;                   // (as gf_codec_master_decode_batch_i32)
    gf_elem_spec elem{};
    elem.type = GF_ELEM_INT;
    elem.scale = 1.0f;
    void *const values[1] = {dValues};
    return recordsDev(c, stream, codecs, nCodecs, &elem, 1, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, dLengths, 0, nullptr, values,
                      dStatus);
}

gf_status gf_tile_record_decode_batch_elems(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems,
                                            int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                                            int verifyChecksum, int32_t *tileIndices, void *const *values, int32_t *status)
{
    gf_status s = elemsArgs(c, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, blob, false, offsets, values, status);
    if (s != GF_OK || nTiles == 0) return s;
    GF_CTX_LOCK(c);
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(c->device));
    const size_t blobBytes = (size_t)offsets[nTiles];
    // staging: blob | offsets | values of element 0, 1, ..., zeroed (an element that fails reads as zeros, not as an earlier call) |
    // statuses | tile indices (a failed record keeps the caller's entry)
    HostStage sg(c);
    int valueP[GF_MAX_ELEMS];
    const int blobP = sg.in(blob, blobBytes, 32), offsetsP = sg.in(offsets, (nTiles + 1) * 8);
    stageElems(sg, STAGE_OUT | STAGE_ZERO, elems, nElems, nTiles * cells, values, valueP);
    const int statusP = sg.out(status, (size_t)nElems * nTiles * 4), indicesP = sg.inout(tileIndices, nTiles * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dValues[GF_MAX_ELEMS];
    sg.ptrs(valueP, nElems, dValues);
    s = recordsDecodeDev(c, c->stream, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, sg.ptr<uint8_t>(blobP), blobBytes,
                         sg.ptr<uint64_t>(offsetsP), nullptr, verifyChecksum, sg.ptr<int32_t>(indicesP), dValues, sg.ptr<int32_t>(statusP));
    return s != GF_OK ? s : sg.end();
}

}  // extern "C"
