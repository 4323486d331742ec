// gvrs_api_records_dev.hip -- tile records and mixed-codec packings decoded where they lie in device memory: what
// gf_tile_record_decode_batch and gf_codec_master_decode_batch_i32 do on the host (walk the framing, verify the CRC-32C, sort the
// packings by codec, narrow shorts, copy raw tiles) as four kernels of gvrs_records.hip around the codecs' device decoders.

#include "gvrs_api_internal.h"

void gf_rec_counts_destroy(PinBuf *p)
{
    if (!p) return;
    p->release();
    delete p;
}

// one codec's share of the batch through its device decoder: packing j = lengths[j] bytes at dBlob + offsets[j]
gf_status decodeSublist(gf_context *c, hipStream_t st, int codec, const RecBatch &b, size_t n, const uint64_t *offsets,
                        const uint32_t *lengths, int32_t *values, int32_t *status)
{
    switch (codec) {
    case GF_CODEC_HUFFMAN:
        return decodeBatchDev(KIND_HUFFMAN, c, st, b.nRows, b.nCols, n, b.dBlob, b.blobBytes, offsets, 0, lengths, values, status, 0);
    case GF_CODEC_CANON_HUFFMAN:
        return decodeBatchDev(KIND_CANON, c, st, b.nRows, b.nCols, n, b.dBlob, b.blobBytes, offsets, 0, lengths, values, status, 0);
    case GF_CODEC_DEFLATE:
        return deflateDecodeDev(c, st, b.nRows, b.nCols, n, b.dBlob, b.blobBytes, offsets, 0, lengths, values, status);
    case GF_CODEC_LSOP12: {
        const size_t resStride = roundUp(gf_lsop12_residual_count(b.nRows, b.nCols), 4);
        gf_status s;
        if ((s = c->dResiduals.ensure(n * resStride * 4 + 16)) != GF_OK) return s;
        if ((s = c->dCoefs.ensure(n * 64 + 16)) != GF_OK) return s;
        if ((s = c->dStatus2.ensure(n * 4 + 16)) != GF_OK) return s;
        return gf_lsop12_decode_batch_i32_dev(c, st, b.nRows, b.nCols, n, b.dBlob, b.blobBytes, offsets, 0, lengths, values, status,
                                              (int32_t *)c->dResiduals.p, resStride, (uint32_t *)c->dCoefs.p, (int32_t *)c->dStatus2.p);
    }
    default: return GF_ERR_ARG;
    }
}

namespace {

// what the host can check without a device
gf_status recArgs(const gf_context *c, const RecBatch &b)
{
    if (!c || !b.dBlob || !b.dOffsets || !b.dValues || !b.dStatus || (!b.codecs && b.nCodecs > 0)) return GF_ERR_ARG;
    if (b.nRows < 1 || b.nCols < 1 || b.nCodecs > 255 || ((uintptr_t)b.dBlob & 3) != 0) return GF_ERR_ARG;
    for (int k = 0; k < b.nCodecs; k++)
        if (b.codecs[k] < GF_CODEC_NONE || b.codecs[k] > GF_CODEC_LSOP12) return GF_ERR_ARG;
    return GF_OK;
}

gf_status recDecodeDev(gf_context *c, void *stream, const RecBatch &b)
{
    if (b.nTiles > 0x7fffffffull) return GF_ERR_UNSUPPORTED;                      // record numbers travel as 32 bits
    const size_t cells = (size_t)b.nRows * (size_t)b.nCols, n = b.nTiles;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = streamOf(c, stream);
    const int nSeg = b.nCodecs + 1;                                               // the codecs, then the standard form
    const size_t nPad = roundUp(n, 4);
    gf_status s;
    if ((s = c->dRecMeta.ensure(nPad * 20 + 16)) != GF_OK) return s;
    if ((s = c->dRecSub.ensure(nPad * 20 + 256 * 4 + 16)) != GF_OK) return s;
    if (!c->hRecCounts) {
        c->hRecCounts = new (std::nothrow) PinBuf();
        if (!c->hRecCounts) return GF_ERR_HIP;
    }
    if ((s = c->hRecCounts->ensure(256 * 4)) != GF_OK) return s;
    uint64_t *starts = (uint64_t *)c->dRecMeta.p;
    uint32_t *lens = (uint32_t *)(starts + nPad), *sizes = lens + nPad;
    int32_t *cls = (int32_t *)(sizes + nPad);
    uint64_t *subOffsets = (uint64_t *)c->dRecSub.p;
    uint32_t *subLengths = (uint32_t *)(subOffsets + nPad), *subDst = subLengths + nPad;
    int32_t *subStatus = (int32_t *)(subDst + nPad);
    uint32_t *dCounts = (uint32_t *)(subStatus + nPad);

    GfRecordParseArgs p{};
    p.blob = b.dBlob;
    p.blobBytes = b.blobBytes;
    p.offsets = b.dOffsets;
    p.lengths = b.dLengths;
    p.nTiles = n;
    // TileElement.java:86-93: bytes per sample * cells, rounded up to a multiple of 4
    p.stdSize = b.dLengths ? 0u : (uint32_t)(b.elemShort ? ((cells * 2 + 3) & ~(size_t)3) : cells * 4);
    p.nCodecs = b.nCodecs;
    uint64_t set[4] = {0, 0, 0, 0};
    for (int k = 0; k < b.nCodecs; k++)
        if (b.codecs[k] != GF_CODEC_NONE) set[k >> 6] |= 1ull << (k & 63);
    p.codecSet0 = set[0], p.codecSet1 = set[1], p.codecSet2 = set[2], p.codecSet3 = set[3];
    p.tileIndices = b.dTileIndices;
    p.starts = starts;
    p.lens = lens;
    p.sizes = sizes;
    p.cls = cls;
    p.status = b.dStatus;
    GF_HIP(gf_launch_record_parse(p, st));
    if (!b.dLengths && b.verifyChecksum) GF_HIP(gf_launch_record_crc32c(b.dBlob, starts, sizes, cls, b.dStatus, n, st));
    GfPartitionArgs q{};
    q.cls = cls;
    q.starts = starts;
    q.lens = lens;
    q.nTiles = n;
    q.nCodecs = b.nCodecs;
    q.subOffsets = subOffsets;
    q.subLengths = subLengths;
    q.subDst = subDst;
    q.counts = dCounts;
    GF_HIP(gf_launch_codec_partition(q, st));
    // the one synchronisation of the call: the host has to know which decoders to launch, and for how many tiles
    const uint32_t *counts = (const uint32_t *)c->hRecCounts->p;
    GF_HIP(hipMemcpyAsync(c->hRecCounts->p, dCounts, (size_t)nSeg * 4, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    size_t nPacked = 0;
    for (int k = 0; k < b.nCodecs; k++) nPacked += counts[k];
    const size_t nStd = counts[b.nCodecs];
    // every record names the same codec (and none failed): the partition is the identity, its decoder writes straight to the caller's arrays
    if (!b.elemShort)
        for (int k = 0; k < b.nCodecs; k++)
            if (counts[k] == n) return decodeSublist(c, st, b.codecs[k], b, n, starts, lens, (int32_t *)b.dValues, b.dStatus);
    if (nPacked && (s = c->dRecTmp.ensure(nPacked * cells * 4 + 64)) != GF_OK) return s;
    int32_t *tmp = (int32_t *)c->dRecTmp.p;
    size_t j0 = 0;
    for (int k = 0; k < b.nCodecs; k++) {                                          // in list order, on the caller's stream
        const size_t nk = counts[k];
        if (!nk) continue;
        s = decodeSublist(c, st, b.codecs[k], b, nk, subOffsets + j0, subLengths + j0, tmp + j0 * cells, subStatus + j0);
        if (s != GF_OK) return s;
        j0 += nk;
    }
    GfTileScatterArgs g{};
    g.blob = b.dBlob;
    g.tmp = tmp;
    g.subStatus = subStatus;
    g.subOffsets = subOffsets;
    g.subDst = subDst;
    g.nPacked = nPacked;
    g.nTotal = nPacked + nStd;
    g.cells = (uint32_t)cells;
    g.elemShort = b.elemShort;
    g.values = b.dValues;
    g.status = b.dStatus;
    GF_HIP(gf_launch_tile_scatter(g, st));
    return GF_OK;
}

}  // namespace

extern "C" {

gf_status gf_codec_master_decode_batch_i32_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, int nRows, int nCols,
                                               size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                                               const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus)
{
    const RecBatch b{codecs, nCodecs, 0, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, dLengths, 0, nullptr, dValues, dStatus};
    if (!dLengths || !codecs || nCodecs < 1) return GF_ERR_ARG;                   // (as gf_codec_master_decode_batch_i32)
    const gf_status s = recArgs(c, b);
    if (s != GF_OK) return s;
    if (nTiles == 0) return GF_OK;
    GF_CTX_LOCK(c);
    return recDecodeDev(c, stream, b);
}

gf_status gf_tile_record_decode_batch_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, int elemType, int nRows,
                                          int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                                          int verifyChecksum, int32_t *dTileIndices, void *dValues, int32_t *dStatus)
{
    if (elemType != GF_ELEM_INT && elemType != GF_ELEM_SHORT) return GF_ERR_ARG;
    const RecBatch b{codecs, nCodecs < 0 ? 0 : nCodecs, elemType == GF_ELEM_SHORT, nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, nullptr,
                     verifyChecksum, dTileIndices, dValues, dStatus};
    const gf_status s = recArgs(c, b);
    if (s != GF_OK) return s;
    if (nTiles == 0) return GF_OK;
    GF_CTX_LOCK(c);
    return recDecodeDev(c, stream, b);
}

}  // extern "C"
