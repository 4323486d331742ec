// gvrs_api_file_update.hip -- GVRS files UPDATED IN PLACE: gf_file_update_begin / _end / _free_list / _plan / _assemble (the
// allocator and the close sequence of gvrs_file_update.h behind a handle and their argument checks; no device, no context),
// gf_file_update_records_dev (records in device memory placed into an image in device memory by the kernels of
// gvrs_file_update.hip), gf_file_update_block_elems_dev (k_file_locate, the block write's pipeline into a buffer of the context,
// then the records form) and gf_file_update_block_elems (the old records looked up on the host, gf_block_write_elems, then the
// assembler).
// Reference: gvrs/GvrsFile.java:443-483, 584-616, gvrs/RecordManager.java:218-490, 864-1017.

#include "gvrs_api_internal.h"
#include "gvrs_file_update.h"

struct gf_file_update {
    GfFileUpdate u;
};

extern "C" {

gf_status gf_file_update_begin(const gf_file *f, const uint8_t *image, size_t imageBytes, gf_file_update **out)
{
    if (!f || !image || !out) return GF_ERR_ARG;
    *out = nullptr;
    gf_file_info info;
    gf_status s = gf_file_get_info(f, &info);
    if (s != GF_OK) return s;
    gf_file_update *h = new (std::nothrow) gf_file_update();
    if (!h) return GF_ERR_CAPACITY;
    if ((s = gfFileUpdateBegin(info, image, imageBytes, h->u)) != GF_OK) {
        delete h;
        return s;
    }
    *out = h;
    return GF_OK;
}

void gf_file_update_end(gf_file_update *u) { delete u; }

gf_status gf_file_update_free_list(const gf_file_update *u, uint64_t *positions, uint64_t *sizes, size_t cap, size_t *nNodes)
{
    if (!u || !nNodes || (cap && (!positions || !sizes))) return GF_ERR_ARG;
    *nNodes = u->u.freePos.size();
    if (*nNodes > cap) return GF_ERR_CAPACITY;
    for (size_t k = 0; k < *nNodes; k++) positions[k] = u->u.freePos[k], sizes[k] = u->u.freeSize[k];
    return GF_OK;
}

gf_status gf_file_update_plan(const gf_file_update *u, const gf_rect *rect, uint64_t *maxImageBytes, uint64_t *freeListCapacity)
{
    if (!u) return GF_ERR_ARG;
    const gf_file_info &i = u->u.info;
    const gf_rect whole{0, 0, i.grid.n_rows_grid, i.grid.n_cols_grid};
    GfBlockGeom g{};
    gf_status s = blockGeom(&i.grid, rect ? rect : &whole, g);
    if (s != GF_OK) return s;
    size_t maxRecord;
    if ((s = fileMaxRecord(i.elems, i.n_elems, g, maxRecord)) != GF_OK) return s;
    gfFileUpdatePlan(u->u, (uint64_t)g.nTileRows * (uint64_t)g.nTileCols, maxRecord, maxImageBytes, freeListCapacity);
    return GF_OK;
}

gf_status gf_file_update_plan_tiles(const gf_file_update *u, size_t nTiles, uint64_t *maxImageBytes, uint64_t *freeListCapacity)
{
    if (!u) return GF_ERR_ARG;
    const gf_file_info &i = u->u.info;
    if ((uint64_t)nTiles > (uint64_t)gfTilesOfGrid(i.grid).count()) return GF_ERR_ARG;   // (no update writes more tiles than the grid has)
    GfBlockGeom g{};
    g.nRowsTile = i.grid.n_rows_tile, g.nColsTile = i.grid.n_cols_tile;
    size_t maxRecord;
    const gf_status s = fileMaxRecord(i.elems, i.n_elems, g, maxRecord);
    if (s != GF_OK) return s;
    gfFileUpdatePlan(u->u, (uint64_t)nTiles, maxRecord, maxImageBytes, freeListCapacity);
    return GF_OK;
}

gf_status gf_file_update_assemble(const gf_file_update *u, uint8_t *image, size_t imageCap, const uint8_t *blob, const uint64_t *offsets,
                                  const int32_t *tileIndices, const int32_t *status, size_t nRecords, int64_t timeModified, int flags,
                                  uint64_t *imageBytes)
{
    if (!u || !image || !imageBytes || (nRecords && (!offsets || !tileIndices))) return GF_ERR_ARG;
    if (blob && nRecords && (uintptr_t)blob < (uintptr_t)image + imageCap && (uintptr_t)blob + offsets[nRecords] > (uintptr_t)image) return GF_ERR_ARG;
    return gfFileUpdateAssemble(u->u, image, imageCap, blob, offsets, tileIndices, status, nRecords, timeModified, flags, imageBytes);
}

}  // extern "C"

const GfFileUpdate &fileUpdateOf(const gf_file_update *u) { return u->u; }

// the records form behind its null checks (the caller holds the context's lock).  dTileStatus: null, or the block form's statuses,
// into which a refused old record puts its tile's verdict
gf_status updateRecordsDev(gf_context *c, const GfFileUpdate &h, uint8_t *dImage, size_t imageCap, const uint8_t *dBlob, const uint64_t *dOffsets,
                                  const int32_t *dTileIndices, const int32_t *dStatus, int32_t *dTileStatus, size_t nRecords, size_t blobBytes,
                                  int64_t timeModified, int flags, size_t listCapacity, uint64_t *dImageBytes, int32_t *dFileStatus)
{
    const gf_file_info &i = h.info;
    if (imageCap < h.imageBytes) return GF_ERR_ARG;
    const size_t need = h.freePos.size() + nRecords + 3, cap = listCapacity ? listCapacity : need;
    if (cap < need) return GF_ERR_ARG;
    if (nRecords > 0x7fffffffull || cap > 0x7fffffffull) return GF_ERR_UNSUPPORTED;
    const uint64_t nTilesGrid = (uint64_t)gfTilesOfGrid(i.grid).count();
    if (gfFileTileDirSize(nTilesGrid, true) > 0x7fffffffull) return GF_ERR_UNSUPPORTED;   // (a record's size is an int32)
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    const size_t nOpened = h.freePos.size();
    // the context's part: state | positions of the records | the list (positions, sizes, prefix sums) | the old entries of the
    // grid's tiles | the records' count per tile | the metadata directory | the tile directory's chunk checksums
    Carve k;
    const size_t stateAt = k.add(sizeof(GfFileUpdateState)), recPosAt = k.add(nRecords * 8), posAt = k.add(cap * 8), sizeAt = k.add(cap * 8);
    const size_t prefixAt = k.add((cap + 1) * 8), gridAt = k.add(nTilesGrid * 8), seenAt = k.add(nTilesGrid * 4), metaDirAt = k.add(h.metaDir.size());
    const size_t chunksAt = k.add((gfFileTileDirSize(nTilesGrid, true) / GF_FILE_CRC_CHUNK + 1) * 4);
    gf_status s = c->dFileUpdate.ensure(k);
    if (s != GF_OK) return s;
    GfFileUpdateArgs a{};
    a.image = dImage;
    a.imageCap = imageCap, a.oldBytes = h.imageBytes;
    a.dir = gfFileDirOf(i), a.nTilesGrid = (int32_t)nTilesGrid;
    a.checksums = i.checksum_enabled ? 1 : 0, a.compression = i.n_codecs > 0 ? 1 : 0, a.forceExtended = (flags & GF_FILE_DIR_EXTENDED) ? 1 : 0;
    a.timeModified = timeModified;
    a.blob = dBlob, a.offsets = dOffsets, a.tiles = dTileIndices, a.status = dStatus, a.tileStatus = dTileStatus;
    a.nRecords = nRecords, a.blobBytes = blobBytes;
    a.state = c->dFileUpdate.at<GfFileUpdateState>(stateAt);
    a.recPos = c->dFileUpdate.at<uint64_t>(recPosAt);
    a.listPos = c->dFileUpdate.at<uint64_t>(posAt), a.listSize = c->dFileUpdate.at<uint64_t>(sizeAt), a.listPrefix = c->dFileUpdate.at<uint64_t>(prefixAt);
    a.listCap = (uint32_t)cap, a.nOpened = (uint32_t)nOpened;
    a.grid = c->dFileUpdate.at<uint64_t>(gridAt);
    a.seen = c->dFileUpdate.at<uint32_t>(seenAt);
    a.metaDir = c->dFileUpdate.at<uint8_t>(metaDirAt);
    a.metaDirBytes = (uint32_t)h.metaDir.size();
    a.chunkCrc = c->dFileUpdate.at<uint32_t>(chunksAt);
    a.imageBytes = dImageBytes, a.fileStatus = dFileStatus;
    // the opened list and the metadata directory travel through the page-locked buffer that a written file's front uses
    if ((s = fileFrontSend(c, st, {{h.freePos.data(), a.listPos, nOpened * 8}, {h.freeSize.data(), a.listSize, nOpened * 8},
                                   {h.metaDir.data(), const_cast<uint8_t *>(a.metaDir), h.metaDir.size()}})) != GF_OK) return s;
    GF_HIP(hipMemsetAsync(a.seen, 0, nTilesGrid * 4, st));
    GF_HIP(gf_launch_file_update(a, st));
    return GF_OK;
}

extern "C" {

gf_status gf_file_update_records_dev(gf_context *c, const gf_file_update *u, uint8_t *dImage, size_t imageCap, const uint8_t *dBlob,
                                     const uint64_t *dOffsets, const int32_t *dTileIndices, const int32_t *dStatus, size_t nRecords,
                                     size_t blobBytes, int64_t timeModified, int flags, size_t listCapacity, uint64_t *dImageBytes,
                                     int32_t *dFileStatus)
{
    if (!c || !u || !dImage || ((uintptr_t)dImage & 7) != 0 || !dImageBytes || !dFileStatus) return GF_ERR_ARG;
    if ((nRecords && (!dOffsets || !dTileIndices)) || (blobBytes && (!dBlob || ((uintptr_t)dBlob & 7) != 0))) return GF_ERR_ARG;
    GF_CTX_LOCK(c);
    return updateRecordsDev(c, u->u, dImage, imageCap, dBlob, dOffsets, dTileIndices, dStatus, nullptr, nRecords, blobBytes, timeModified, flags,
                            listCapacity, dImageBytes, dFileStatus);
}

gf_status gf_file_update_block_elems_dev(gf_context *c, const gf_file_update *u, const gf_rect *rect, const void *const *dBlocks, int flags,
                                         int64_t timeModified, uint8_t *dImage, size_t imageCap, uint64_t *dImageBytes, int32_t *dFileStatus,
                                         int32_t *dTileIndices, int32_t *dStatus, uint8_t *dCodecUsed)
{
    if (!c || !u || !dImage || ((uintptr_t)dImage & 7) != 0 || !dImageBytes || !dFileStatus) return GF_ERR_ARG;
    const GfFileUpdate &h = u->u;
    const gf_file_info &i = h.info;
    if (imageCap < h.imageBytes) return GF_ERR_ARG;
    for (int k = 0; k < i.n_codecs; k++)
        if (i.codecs[k] == GF_CODEC_UNKNOWN) return GF_ERR_UNSUPPORTED;
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    // (the places of blob and offsets are taken by the image: the block write's checks only look at them for null)
    gf_status s = blockWriteArgs(c, i.codecs, i.n_codecs, i.elems, nullptr, i.n_elems, &i.grid, rect, dBlocks, 0, nullptr, nullptr, dImage, imageCap,
                                 (const uint64_t *)dImage, dTileIndices, dStatus, true, g, cut);
    if (s != GF_OK) return s;
    if (!deviceList(i.codecs, i.n_codecs, i.elems, i.n_elems)) return GF_ERR_UNSUPPORTED;
    const size_t T = (size_t)g.nTileRows * (size_t)g.nTileCols;
    size_t maxRecord;
    if ((s = fileMaxRecord(i.elems, i.n_elems, g, maxRecord)) != GF_OK) return s;
    // Only a rectangle whose four sides lie on tile seams needs no old cell: it decodes nothing and never synchronises.  A tile that
    // the grid's edge cuts keeps its old cells beyond the grid, as the reference's tile does, so a rectangle that ends at such an edge
    // takes the old records' route.
    const bool aligned = g.row0 % g.nRowsTile == 0 && g.col0 % g.nColsTile == 0 && (g.row0 + g.nRows) % g.nRowsTile == 0 &&
                         (g.col0 + g.nCols) % g.nColsTile == 0;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    Carve kb;
    const size_t blobAt = kb.add(T * maxRecord), offsetsAt = kb.add((T + 1) * 8);
    if ((s = c->dFileUpdateBlob.ensure(kb)) != GF_OK) return s;
    uint8_t *dBlob = c->dFileUpdateBlob.at<uint8_t>(blobAt);
    uint64_t *dOffsets = c->dFileUpdateBlob.at<uint64_t>(offsetsAt);
    const uint64_t *dStarts = nullptr, *dEnds = nullptr;
    if (!aligned) {
        // the old records of the rectangle's tiles where they lie in the image (k_file_locate): a dense list, a tile without a
        // record or with a refused entry as an empty extent, which names no tile and leaves its slot a new tile to the merge
        GfFileLocateArgs a;
        if ((s = fileLocateDev(c, st, i, dImage, (size_t)h.imageBytes, g, nullptr, a)) != GF_OK) return s;
        dStarts = a.starts, dEnds = a.ends;
    }
    s = blockWriteDev(c, st, i.codecs, i.n_codecs, i.elems, i.n_elems, g, cut, dBlocks, aligned ? 0 : T, aligned ? nullptr : dImage,
                      aligned ? 0 : (size_t)h.imageBytes, dStarts, i.checksum_enabled, i.checksum_enabled, dBlob, T * maxRecord, dOffsets, dTileIndices,
                      dCodecUsed, dStatus, dEnds);
    if (s != GF_OK) return s;
    // the allocator takes the records in row-major order of the rectangle's tiles and judges every old record's head itself: a
    // wholly covered tile with a damaged body is overwritten, one with a damaged size word keeps GF_ERR_FORMAT and stays
    return updateRecordsDev(c, h, dImage, imageCap, dBlob, dOffsets, dTileIndices, dStatus, dStatus, T, T * maxRecord, timeModified, flags, 0,
                            dImageBytes, dFileStatus);
}

gf_status gf_file_update_block_elems(gf_context *c, const gf_file_update *u, const gf_rect *rect, const void *const *blocks, int flags,
                                     int64_t timeModified, uint8_t *image, size_t imageCap, uint64_t *imageBytes, int32_t *tileIndices,
                                     int32_t *status, uint8_t *codecUsed)
{
    if (!c || !u || !rect || !blocks || !image || !imageBytes || !tileIndices || !status) return GF_ERR_ARG;
    *imageBytes = 0;
    const gf_file_info &i = u->u.info;
    if (imageCap < u->u.imageBytes) return GF_ERR_ARG;
    for (int k = 0; k < i.n_codecs; k++)
        if (i.codecs[k] == GF_CODEC_UNKNOWN) return GF_ERR_UNSUPPORTED;
    GfBlockGeom g{};
    gf_status s = blockGeom(&i.grid, rect, g);
    if (s != GF_OK) return s;
    const size_t T = (size_t)g.nTileRows * (size_t)g.nTileCols;
    size_t maxRecord;
    if ((s = fileMaxRecord(i.elems, i.n_elems, g, maxRecord)) != GF_OK) return s;
    // The old records of the rectangle's tiles, looked up and judged by their heads: a tile whose entry or head is refused keeps
    // its verdict and stays as it is.  The block write merges the old cells of partly covered tiles and decodes and ignores the others.
    std::vector<int32_t> verdict(T, GF_OK);
    std::vector<uint8_t> oldBlob;
    std::vector<uint64_t> oldOffsets(1, 0);
    gfFileLocateRect(gfFileDirOf(i), image, u->u.imageBytes, g.tileRow0, g.tileCol0, g.nTileRows, g.nTileCols, [&](size_t j, gf_status v, uint64_t pos, uint32_t) {
        uint64_t size = 0;
        if (v == GF_OK && pos != 0) v = gfFsRecordHead(u->u.imageBytes, i.content_pos, pos, GF_FILE_REC_TILE, 24, &size, GfLoadLe{image});
        verdict[j] = v;
        if (v == GF_OK && pos != 0) {
            oldBlob.insert(oldBlob.end(), image + pos - 8, image + pos - 8 + size);
            oldOffsets.push_back(oldBlob.size());
        }
    });
    const size_t nOld = oldOffsets.size() - 1;
    std::vector<uint8_t> blob(T * maxRecord + 16);
    std::vector<uint64_t> offsets(T + 1, 0);
    s = gf_block_write_elems(c, i.codecs, i.n_codecs, i.elems, nullptr, i.n_elems, &i.grid, rect, blocks, nOld, nOld ? oldBlob.data() : nullptr,
                             nOld ? oldOffsets.data() : nullptr, i.checksum_enabled, i.checksum_enabled, blob.data(), T * maxRecord, offsets.data(),
                             tileIndices, codecUsed, status);
    if (s == GF_ERR_ARG || s == GF_ERR_UNSUPPORTED || s == GF_ERR_HIP || s == GF_ERR_CAPACITY) return s;   // (not a tile's verdict)
    gf_status first = GF_OK;
    for (size_t j = 0; j < T; j++) {
        if (verdict[j] < 0) status[j] = verdict[j];
        if (status[j] < 0 && first == GF_OK) first = (gf_status)status[j];
    }
    s = gfFileUpdateAssemble(u->u, image, imageCap, blob.data(), offsets.data(), tileIndices, status, T, timeModified, flags, imageBytes);
    return s != GF_OK ? s : first;                                // (a refusal of the whole update comes before a tile's status)
}

}  // extern "C"
