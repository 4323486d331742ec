// gvrs_api_file_write.hip -- GVRS files WRITTEN: gf_file_write_plan and gf_file_assemble (the emitters of gvrs_file_emit.h behind
// their argument checks; no device, no context), gf_file_write_block_elems_dev (the host emits the header and metadata records
// to the image's front, the block write's pipeline of gvrs_api_blocks_write.hip lays the records straight into the image, the
// kernels of gvrs_file_write.hip write the directories and finish the header) and gf_file_write_block_elems (gf_block_write_elems
// into the caller's image, then the assembler around the records where they lie).
// Reference: gvrs/GvrsFile.java:239-300, 584-616, gvrs/RecordManager.java:670-719, 864-883, 991-1017.

#include "gvrs_api_internal.h"
#include "gvrs_file_emit.h"

namespace {

// the facts and metadata checked; kinds[255] and ranges[GF_MAX_ELEMS] as the block write takes them
gf_status fileWriteFacts(const gf_file_facts *f, const gf_file_metadata *m, int nMeta, int *kinds, gf_elem_range *ranges)
{
    gf_status s = gfFileFactsCheck(f, kinds);
    if (s != GF_OK) return s;
    if ((s = gfFileMetadataCheck(m, nMeta)) != GF_OK) return s;
    for (int e = 0; e < f->n_elems; e++) {
        if (f->elems[e].type == GF_ELEM_ICF && (f->elems[e].scale == 0.0f || std::isnan(f->elems[e].scale))) return GF_ERR_ARG;
        ranges[e] = gfFileElemRange(f->elems[e], f->elem_facts ? &f->elem_facts[e] : nullptr);
    }
    return GF_OK;
}

gf_rect wholeGrid(const gf_grid_spec &g) { return gf_rect{0, 0, g.n_rows_grid, g.n_cols_grid}; }

}  // namespace

// The parts are copied into the page-locked buffer and from there with hipMemcpyAsync.  The one wait of such a call: an EARLIER
// call's copies must have left that buffer.
gf_status fileFrontSend(gf_context *c, hipStream_t st, std::initializer_list<FileFrontPart> parts)
{
    Carve h, at;
    for (const FileFrontPart &p : parts) h.add(p.bytes);
    if (h.total == 0) return GF_OK;
    if (!c->fileFrontDone) GF_HIP(hipEventCreateWithFlags(&c->fileFrontDone, hipEventDisableTiming));
    GF_HIP(hipEventSynchronize(c->fileFrontDone));
    const gf_status s = c->hFileFront.ensure(h, 16);
    if (s != GF_OK) return s;
    for (const FileFrontPart &p : parts) {
        uint8_t *via = c->hFileFront.at<uint8_t>(at.add(p.bytes));
        if (p.bytes == 0) continue;
        memcpy(via, p.host, p.bytes);
        GF_HIP(hipMemcpyAsync(p.dev, via, p.bytes, hipMemcpyHostToDevice, st));
    }
    GF_HIP(hipEventRecord(c->fileFrontDone, st));
    return GF_OK;
}

extern "C" {

gf_status gf_file_write_plan(const gf_file_facts *facts, const gf_file_metadata *metadata, int nMeta, const gf_rect *rect, int flags,
                             uint64_t *firstRecordPos, uint64_t *maxImageBytes)
{
    int kinds[255];
    gf_elem_range ranges[GF_MAX_ELEMS];
    gf_status s = fileWriteFacts(facts, metadata, nMeta, kinds, ranges);
    if (s != GF_OK) return s;
    const gf_rect whole = wholeGrid(facts->grid);
    GfBlockGeom g{};
    if ((s = blockGeom(&facts->grid, rect ? rect : &whole, g)) != GF_OK) return s;
    size_t maxRecord;
    if ((s = fileMaxRecord(facts->elems, facts->n_elems, g, maxRecord)) != GF_OK) return s;
    GfFileFront w;
    gfFileEmitFront(*facts, metadata, nMeta, w);
    gfFilePlan(w, (uint64_t)g.nTileRows * (uint64_t)g.nTileCols, maxRecord, flags, firstRecordPos, maxImageBytes);
    return GF_OK;
}

gf_status gf_file_assemble(const gf_file_facts *facts, const gf_file_metadata *metadata, int nMeta, int flags, const uint8_t *blob,
                           const uint64_t *offsets, const int32_t *tileIndices, size_t nRecords, uint8_t *image, size_t imageCap,
                           uint64_t *imageBytes)
{
    int kinds[255];
    gf_elem_range ranges[GF_MAX_ELEMS];
    const gf_status s = fileWriteFacts(facts, metadata, nMeta, kinds, ranges);
    if (s != GF_OK) return s;
    return gfFileAssemble(*facts, metadata, nMeta, flags, blob, offsets, tileIndices, nRecords, image, imageCap, imageBytes);
}

gf_status gf_file_write_block_elems_dev(gf_context *c, const gf_file_facts *facts, const gf_file_metadata *metadata, int nMeta,
                                        const gf_rect *rect, const void *const *dBlocks, int flags, uint8_t *dImage, size_t imageCap,
                                        uint64_t *dImageBytes, int32_t *dFileStatus, int32_t *dTileIndices, int32_t *dStatus,
                                        uint8_t *dCodecUsed)
{
    int kinds[255];
    gf_elem_range ranges[GF_MAX_ELEMS];
    gf_status s = fileWriteFacts(facts, metadata, nMeta, kinds, ranges);
    if (s != GF_OK) return s;
    if (!dImage || ((uintptr_t)dImage & 7) != 0 || !dImageBytes || !dFileStatus) return GF_ERR_ARG;
    GfFileFront w;
    gfFileEmitFront(*facts, metadata, nMeta, w);
    const uint64_t p0 = w.firstRecordPos();
    const size_t blobCap = imageCap > p0 ? imageCap - (size_t)p0 : 0;
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    // (the offsets' place is taken by the image: the block write's checks only look at it for null)
    s = blockWriteArgs(c, kinds, facts->n_codecs, facts->elems, ranges, facts->n_elems, &facts->grid, rect, dBlocks, 0, nullptr, nullptr, dImage + p0,
                       blobCap, (const uint64_t *)dImage, dTileIndices, dStatus, true, g, cut);
    if (s != GF_OK) return s;
    if (!deviceList(kinds, facts->n_codecs, facts->elems, facts->n_elems)) return GF_ERR_UNSUPPORTED;
    const size_t nOut = (size_t)g.nTileRows * (size_t)g.nTileCols;
    if (gfFileTileDirSize(nOut, true) > 0x7fffffffull) return GF_ERR_UNSUPPORTED;     // (a record's size is an int32)
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    // the context's part: the kernels' state | the records' offsets | the metadata directory | the directory's chunk checksums
    Carve k;
    const size_t stateAt = k.add(sizeof(GfFileWriteState)), offsetsAt = k.add((nOut + 1) * 8), metaDirAt = k.add(w.metaDir.size());
    const size_t chunksAt = k.add((gfFileTileDirSize(nOut, true) / GF_FILE_CRC_CHUNK + 1) * 4);
    if ((s = c->dFileWrite.ensure(k)) != GF_OK) return s;
    GfFileWriteArgs a{};
    a.image = dImage;
    a.imageCap = imageCap;
    a.firstRecordPos = p0;
    a.contentPos = w.contentPos;
    a.state = c->dFileWrite.at<GfFileWriteState>(stateAt);
    uint64_t *dOffsets = c->dFileWrite.at<uint64_t>(offsetsAt);
    a.offsets = dOffsets;
    a.metaDir = c->dFileWrite.at<uint8_t>(metaDirAt);
    a.metaDirBytes = (uint32_t)w.metaDir.size();
    a.chunkCrc = c->dFileWrite.at<uint32_t>(chunksAt);
    a.checksums = facts->checksum_enabled ? 1 : 0;
    a.forceExtended = (flags & GF_FILE_DIR_EXTENDED) ? 1 : 0;
    a.tileRow0 = g.tileRow0, a.tileCol0 = g.tileCol0, a.nTileRows = g.nTileRows, a.nTileCols = g.nTileCols;
    a.imageBytes = dImageBytes;
    a.fileStatus = dFileStatus;
    GF_HIP(hipMemsetAsync(a.state, 0, sizeof(GfFileWriteState), st));
    // The front -- the header record and the metadata records without the file head (k_file_finish writes it, and only into an image
    // that fits), and the metadata directory.  A short one travels in k_file_finish's arguments.  A long one (large metadata) is
    // copied now, as far as the image reaches, through the context's page-locked buffer (fileFrontSend).
    const bool inArgs = p0 - 16 + w.metaDir.size() <= GF_FILE_FRONT_ARG_BYTES;
    std::vector<uint8_t> frontArg;
    if (inArgs) {
        frontArg.assign(w.front.begin() + 16, w.front.end());
        frontArg.insert(frontArg.end(), w.metaDir.begin(), w.metaDir.end());
    } else {
        const size_t frontBytes = (size_t)std::min<uint64_t>(p0, imageCap);
        if ((s = fileFrontSend(c, st, {{w.front.data() + 16, dImage + 16, frontBytes > 16 ? frontBytes - 16 : 0},
                                       {w.metaDir.data(), const_cast<uint8_t *>(a.metaDir), w.metaDir.size()}})) != GF_OK) return s;
    }
    s = blockWriteDev(c, st, kinds, facts->n_codecs, facts->elems, facts->n_elems, g, cut, dBlocks, 0, nullptr, 0, nullptr, 0, a.checksums, dImage + p0,
                      blobCap, dOffsets, dTileIndices, dCodecUsed, dStatus);
    if (s != GF_OK) return s;
    GF_HIP(gf_launch_file_write(a, inArgs ? frontArg.data() : nullptr, st));
    return GF_OK;
}

gf_status gf_file_write_block_elems(gf_context *c, const gf_file_facts *facts, const gf_file_metadata *metadata, int nMeta, const gf_rect *rect,
                                    const void *const *blocks, int flags, uint8_t *image, size_t imageCap, uint64_t *imageBytes,
                                    int32_t *tileIndices, int32_t *status, uint8_t *codecUsed)
{
    int kinds[255];
    gf_elem_range ranges[GF_MAX_ELEMS];
    gf_status s = fileWriteFacts(facts, metadata, nMeta, kinds, ranges);
    if (s != GF_OK) return s;
    if (!imageBytes || !tileIndices || !status || (!image && imageCap)) return GF_ERR_ARG;
    *imageBytes = 0;
    GfBlockGeom g{};
    if ((s = blockGeom(&facts->grid, rect, g)) != GF_OK) return s;
    const size_t nOut = (size_t)g.nTileRows * (size_t)g.nTileCols;
    GfFileFront w;
    gfFileEmitFront(*facts, metadata, nMeta, w);
    // the records go where the image holds them: row-major order of the rectangle's tiles is the order of the block write's output
    const uint64_t p0 = w.firstRecordPos();
    const size_t blobCap = imageCap > p0 ? imageCap - (size_t)p0 : 0;
    uint8_t *blob = blobCap ? image + p0 : nullptr;
    std::vector<uint64_t> offsets(nOut + 1, 0);
    s = gf_block_write_elems(c, kinds, facts->n_codecs, facts->elems, ranges, facts->n_elems, &facts->grid, rect, blocks, 0, nullptr, nullptr, 0,
                             facts->checksum_enabled, blob, blobCap, offsets.data(), tileIndices, codecUsed, status);
    if (s == GF_ERR_ARG || s == GF_ERR_UNSUPPORTED || s == GF_ERR_HIP) return s;     // (not a tile's verdict: the arrays are not filled in)
    gf_status first = GF_OK;
    for (size_t t = 0; t < nOut && first == GF_OK; t++)
        if (status[t] < 0) first = (gf_status)status[t];
    // an image too small for the records: the assembler says what it needs and writes nothing
    const bool fits = offsets[nOut] <= blobCap;
    s = gfFileAssemble(*facts, metadata, nMeta, flags, blob, offsets.data(), tileIndices, nOut, image, fits ? imageCap : 0, imageBytes);
    return first != GF_OK ? first : s;
}

}  // extern "C"
