// gvrs_api_blocks.hip -- grid blocks: what GvrsElement.readBlock delivers, a rectangle of the raster assembled from the tiles it
// touches with the fill value where the file holds none, and its inverse, a raster cut into tiles for the encoders.  The gather
// alone (gf_block_from_tiles_dev), the cut (gf_tiles_from_block_dev), and records -> blocks (gf_block_read_elems[_dev]): the
// driver of gvrs_api_records_dev.hip into a temporary of the context, then k_block_slots and k_block_gather (gvrs_blocks.hip).
// Reference: gvrs/GvrsElement.java:298-404, gvrs/TileAccessIndices.java:79-88, gvrs/GvrsFileSpecification.java:423-424.

#include "gvrs_api_internal.h"

// what the host can check of the geometry; fills g
gf_status blockGeom(const gf_grid_spec *grid, const gf_rect *rect, GfBlockGeom &g)
{
    if (!grid || !rect) return GF_ERR_ARG;
    if (grid->n_rows_grid < 1 || grid->n_cols_grid < 1 || grid->n_rows_tile < 1 || grid->n_cols_tile < 1) return GF_ERR_ARG;
    if (rect->row0 < 0 || rect->col0 < 0 || rect->n_rows < 1 || rect->n_cols < 1) return GF_ERR_ARG;
    if ((int64_t)rect->row0 + rect->n_rows > grid->n_rows_grid || (int64_t)rect->col0 + rect->n_cols > grid->n_cols_grid) return GF_ERR_ARG;
    const int64_t nRowsOfTiles = ((int64_t)grid->n_rows_grid + grid->n_rows_tile - 1) / grid->n_rows_tile;
    const int64_t nColsOfTiles = ((int64_t)grid->n_cols_grid + grid->n_cols_tile - 1) / grid->n_cols_tile;
    if (nRowsOfTiles * nColsOfTiles > 0x7fffffffll) return GF_ERR_UNSUPPORTED;
    if ((uint64_t)grid->n_rows_tile * (uint64_t)grid->n_cols_tile >= (1ull << 28)) return GF_ERR_UNSUPPORTED;      // (as the records' driver)
    g.nRowsTile = grid->n_rows_tile, g.nColsTile = grid->n_cols_tile;
    g.nColsOfTiles = (int32_t)nColsOfTiles, g.nTilesGrid = (int32_t)(nRowsOfTiles * nColsOfTiles);
    g.row0 = rect->row0, g.col0 = rect->col0, g.nRows = rect->n_rows, g.nCols = rect->n_cols;
    g.tileRow0 = rect->row0 / grid->n_rows_tile, g.tileCol0 = rect->col0 / grid->n_cols_tile;
    g.nTileRows = (rect->row0 + rect->n_rows - 1) / grid->n_rows_tile - g.tileRow0 + 1;
    g.nTileCols = (rect->col0 + rect->n_cols - 1) / grid->n_cols_tile - g.tileCol0 + 1;
    return GF_OK;
}

// ARG before UNSUPPORTED, whichever check finds it
gf_status firstOf(gf_status a, gf_status b)
{
    if (a == GF_ERR_ARG || b == GF_ERR_ARG) return GF_ERR_ARG;
    return a != GF_OK ? a : b;
}

namespace {

// slot table pre-set to -1, k_block_slots over the records' tile indices, k_block_gather; elems: the device table of nElems
// entries, or null for the one element `one`.  Enqueues only (the slot table grows before the first launch).
gf_status gatherDev(gf_context *c, hipStream_t st, const GfBlockGeom &g, size_t nRecords, const int32_t *dTileIndices, const GfBlockElem *dElems,
                    const GfBlockElem &one, int nElems)
{
    const size_t nSlots = (size_t)g.nTileRows * (size_t)g.nTileCols;
    gf_status s;
    if ((s = c->dBlockSlots.ensure(nSlots * 4 + 16)) != GF_OK) return s;
    GF_HIP(hipMemsetAsync(c->dBlockSlots.p, 0xff, nSlots * 4, st));
    GfBlockSlotsArgs p{};
    p.tileIndices = dTileIndices;
    p.nRecords = nRecords;
    p.slots = (int32_t *)c->dBlockSlots.p;
    p.g = g;
    GF_HIP(gf_launch_block_slots(p, st));
    GfBlockGatherArgs q{};
    q.slots = (const int32_t *)c->dBlockSlots.p;
    q.elems = dElems;
    q.one = one;
    q.nElems = nElems;
    q.g = g;
    GF_HIP(gf_launch_block_gather(q, st));
    return GF_OK;
}

}  // namespace

// the fill value's bits per element; a SHORT's must be an int16
gf_status elemFills(const gf_elem_spec *elems, int nElems, uint32_t *fill)
{
    for (int e = 0; e < nElems; e++) {
        const int type = elems[e].type;
        if (type == GF_ELEM_FLOAT || type == GF_ELEM_ICF) memcpy(&fill[e], &elems[e].fill_f, 4);
        else {
            if (type == GF_ELEM_SHORT && (elems[e].fill_i < -32768 || elems[e].fill_i > 32767)) return GF_ERR_ARG;
            fill[e] = (uint32_t)elems[e].fill_i;
        }
    }
    return GF_OK;
}

// what the host can check of a block read's arguments (gvrs_api_downsample.hip shares it); fills g and fill
gf_status blockReadArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const gf_grid_spec *grid,
                        const gf_rect *rect, size_t nRecords, const uint8_t *blob, bool blobOnDevice, const uint64_t *offsets,
                        void *const *blocks, const int32_t *status, GfBlockGeom &g, uint32_t *fill)
{
    if (!grid || !rect) return GF_ERR_ARG;
    const gf_status sa = elemsArgs(c, codecs, nCodecs, elems, nElems, grid->n_rows_tile, grid->n_cols_tile, nRecords, blob, blobOnDevice, offsets,
                                   blocks, status);
    if (sa == GF_ERR_ARG) return sa;
    const gf_status sg = firstOf(blockGeom(grid, rect, g), elemFills(elems, nElems, fill));
    return firstOf(sg, sa);
}

// records in device memory -> one block per element in device memory (the caller holds the lock and has checked the arguments).
// dEnds, dVerdict (both null, or both given: a file image, gvrs_api_file.hip): record t = [dOffsets[t], dEnds[t]), and behind the
// records' pipeline k_file_status puts the verdict of every slot that was not located into the statuses.
gf_status blockReadDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const GfBlockGeom &g,
                       const uint32_t *fill, size_t n, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets, int verifyChecksum,
                       void *const *dBlocks, int32_t *dStatus, const uint64_t *dEnds, const int32_t *dVerdict)
{
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = streamOf(c, stream);
    const size_t cells = (size_t)g.nRowsTile * (size_t)g.nColsTile;
    // the temporary: n_elems arrays of n_records * cells items; the gather's element table and the records' tile indices
    Carve idx;
    void *dValues[GF_MAX_ELEMS];
    const size_t tableAt = idx.add(GF_MAX_ELEMS * sizeof(GfBlockElem)), indicesAt = idx.add(n * 4);
    gf_status s;
    if ((s = elemArrays(c->dBlockTmp, elems, nElems, n * cells, dValues)) != GF_OK) return s;
    if ((s = c->dBlockIdx.ensure(idx)) != GF_OK) return s;
    GfBlockElem *dElems = c->dBlockIdx.at<GfBlockElem>(tableAt);
    int32_t *dIndices = c->dBlockIdx.at<int32_t>(indicesAt);
    GfBlockElem table[GF_MAX_ELEMS] = {};
    for (int e = 0; e < nElems; e++) {
        table[e].tiles = dValues[e];
        table[e].block = dBlocks[e];
        table[e].status = dStatus + (size_t)e * n;
        table[e].fillBits = fill[e];
        table[e].itemBytes = (uint32_t)elemItemBytes(elems[e].type);
    }
    // (a source on this stack: the driver synchronises the stream below; without records this call does so itself, at its end)
    GF_HIP(hipMemcpyAsync(dElems, table, (size_t)nElems * sizeof(GfBlockElem), hipMemcpyHostToDevice, st));
    if (n) {
        GF_HIP(hipMemsetAsync(dIndices, 0xff, n * 4, st));                      // (the driver leaves a failed record's entry alone: -1 places nothing)
        s = recordsDecodeDev(c, stream, codecs, nCodecs, elems, nElems, g.nRowsTile, g.nColsTile, n, dBlob, blobBytes, dOffsets, nullptr,
                             verifyChecksum, dIndices, dValues, dStatus, dEnds);
        if (s != GF_OK) return s;
        if (dVerdict) GF_HIP(gf_launch_file_status(dVerdict, dStatus, n, nElems, st));
    }
    if ((s = gatherDev(c, st, g, n, dIndices, dElems, table[0], nElems)) != GF_OK) return s;
    if (!n) GF_HIP(hipStreamSynchronize(st));                                    // (the call's one synchronisation, which the driver did not make)
    return GF_OK;
}

extern "C" {

gf_status gf_block_from_tiles_dev(gf_context *c, void *stream, const gf_grid_spec *grid, const gf_rect *rect, int elemType, uint32_t fillBits,
                                  size_t nTiles, const int32_t *dTileIndices, const int32_t *dTileStatus, const void *dTiles, void *dBlock)
{
    if (!c || !dTileIndices || !dTiles || !dBlock || elemType < GF_ELEM_INT || elemType > GF_ELEM_ICF) return GF_ERR_ARG;
    GfBlockGeom g{};
    const gf_status s = blockGeom(grid, rect, g);
    if (s != GF_OK) return s;
    if (nTiles > 0x7fffffffull) return GF_ERR_UNSUPPORTED;                        // record numbers travel as int32
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    GfBlockElem one{};
    one.tiles = dTiles;
    one.block = dBlock;
    one.status = dTileStatus;
    one.fillBits = fillBits;
    one.itemBytes = (uint32_t)elemItemBytes(elemType);
    return gatherDev(c, streamOf(c, stream), g, nTiles, dTileIndices, nullptr, one, 1);
}

gf_status gf_tiles_from_block_dev(gf_context *c, void *stream, const gf_grid_spec *grid, const gf_rect *rect, int elemType, uint32_t fillBits,
                                  int keepOutside, const void *dBlock, size_t nTiles, const int32_t *dTileIndices, void *dTiles, int32_t *dStatus)
{
    if (!c || !dBlock || !dTileIndices || !dTiles || elemType < GF_ELEM_INT || elemType > GF_ELEM_ICF) return GF_ERR_ARG;
    GfBlockGeom g{};
    const gf_status s = blockGeom(grid, rect, g);
    if (s != GF_OK) return s;
    if (nTiles > 0x7fffffffull) return GF_ERR_UNSUPPORTED;
    if (nTiles == 0) return GF_OK;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    GfGridCutArgs a{};
    a.block = dBlock;
    a.tiles = dTiles;
    a.tileIndices = dTileIndices;
    a.status = dStatus;
    a.nTiles = nTiles;
    a.fillBits = fillBits;
    a.itemBytes = (uint32_t)elemItemBytes(elemType);
    a.keepOutside = keepOutside;
    a.g = g;
    GF_HIP(gf_launch_grid_cut(a, streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_block_read_elems_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems,
                                  const gf_grid_spec *grid, const gf_rect *rect, size_t nRecords, const uint8_t *dBlob, size_t blobBytes,
                                  const uint64_t *dOffsets, int verifyChecksum, void *const *dBlocks, int32_t *dStatus)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    const gf_status s = blockReadArgs(c, codecs, nCodecs, elems, nElems, grid, rect, nRecords, dBlob, true, dOffsets, dBlocks, dStatus, g, fill);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    return blockReadDev(c, stream, codecs, nCodecs, elems, nElems, g, fill, nRecords, dBlob, blobBytes, dOffsets, verifyChecksum, dBlocks, dStatus);
}

gf_status gf_block_read_elems(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const gf_grid_spec *grid,
                              const gf_rect *rect, size_t nRecords, const uint8_t *blob, const uint64_t *offsets, int verifyChecksum,
                              void *const *blocks, int32_t *status)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    gf_status s = blockReadArgs(c, codecs, nCodecs, elems, nElems, grid, rect, nRecords, blob, false, offsets, blocks, status, g, fill);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const size_t blobBytes = nRecords ? (size_t)offsets[nRecords] : 0;
    // staging: blob | offsets | the block of element 0, 1, ... | statuses
    HostStage sg(c);
    int blockP[GF_MAX_ELEMS];
    const int blobP = sg.in(blob, blobBytes, 32), offsetsP = sg.in(offsets, nRecords ? (nRecords + 1) * 8 : 0);
    stageElems(sg, STAGE_OUT, elems, nElems, (size_t)g.nRows * (size_t)g.nCols, blocks, blockP);
    const int statusP = sg.out(status, (size_t)nElems * nRecords * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dBlocks[GF_MAX_ELEMS];
    sg.ptrs(blockP, nElems, dBlocks);
    s = blockReadDev(c, c->stream, codecs, nCodecs, elems, nElems, g, fill, nRecords, sg.ptr<uint8_t>(blobP), blobBytes, sg.ptr<uint64_t>(offsetsP),
                     verifyChecksum, dBlocks, sg.ptr<int32_t>(statusP));
    return s != GF_OK ? s : sg.end();
}

}  // extern "C"
