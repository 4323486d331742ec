// gvrs_api_blocks_write.hip -- a block WRITTEN: raster in, tile records out.  gf_block_write_elems[_dev] composes what a caller had to
// do by hand: the rectangle of tiles a rectangle touches (gf_block_tile_rect), the old records of partly covered tiles decoded and
// merged (the records driver of gvrs_api_records_dev.hip, k_block_slots), every element cut into tiles with the tile cache's range
// checks, float-to-code conversion and "has valid data" verdict (k_block_cut_elems, k_block_write_verdict: gvrs_blocks_write.hip),
// and the record writer of gvrs_api_records_enc.hip with that verdict as its pre-status.
// Reference: gvrs/TileElement{Int,Short,Float,IntCodedFloat}.java (setValue, setIntValue, hasValidData), gvrs/RasterTile.java:215-222,
// gvrs/RecordManager.java:386-490 (writeTile; :413-419 a tile without valid data), gvrs/GvrsElementSpecification*.java (the ranges).

#include "gvrs_api_internal.h"

#include <climits>

namespace {

uint32_t floatBits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

}  // namespace

// the cut's description of every element (block, tiles and old tiles are set later); GF_ERR_ARG for a range with min > max or a NaN
// bound.  ranges == null: the default constructors of GvrsElementSpecification{Int,Short,Float,IntCodedFloat}.
// (gvrs_api_file_points.hip shares it)
gf_status cutElems(const gf_elem_spec *elems, const gf_elem_range *ranges, int nElems, GfBlockCutElem *t)
{
    for (int e = 0; e < nElems; e++) {
        const gf_elem_spec &s = elems[e];
        GfBlockCutElem &d = t[e];
        d = GfBlockCutElem{};
        d.type = s.type;
        d.scale = s.scale, d.offset = s.offset;
        if (s.type == GF_ELEM_INT || s.type == GF_ELEM_SHORT) {
            int32_t lo = s.type == GF_ELEM_INT ? INT_MIN + 1 : -32767, hi = s.type == GF_ELEM_INT ? INT_MAX : 32767;
            if (ranges) {
                lo = ranges[e].min_i, hi = ranges[e].max_i;
                if (lo > hi) return GF_ERR_ARG;
            }
            d.fillBits = s.type == GF_ELEM_SHORT ? (uint32_t)s.fill_i & 0xffffu : (uint32_t)s.fill_i;
            d.minBits = (uint32_t)lo, d.maxBits = (uint32_t)hi;
        } else {
            float lo = -INFINITY, hi = INFINITY;
            if (s.type == GF_ELEM_ICF) {                                        // GvrsElementSpecificationIntCodedFloat.java:113-116, in float32
                const float a = (float)(INT_MIN + 1) / s.scale, b = (float)(INT_MAX - 1) / s.scale;
                lo = a + s.offset, hi = b + s.offset;
            }
            if (ranges) {
                lo = ranges[e].min_f, hi = ranges[e].max_f;
                if (std::isnan(lo) || std::isnan(hi) || lo > hi) return GF_ERR_ARG;
            }
            d.fillBits = s.type == GF_ELEM_ICF ? (uint32_t)s.fill_i : floatBits(s.fill_f);
            d.fillFBits = floatBits(s.fill_f);
            d.minBits = floatBits(lo), d.maxBits = floatBits(hi);
        }
    }
    return GF_OK;
}

// what the host can check, before the context or a device is looked at; fills g and the cut's element descriptions
// (gvrs_api_image.hip shares it)
gf_status blockWriteArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, const gf_elem_range *ranges, int nElems,
                         const gf_grid_spec *grid, const gf_rect *rect, const void *const *blocks, size_t nOld, const uint8_t *oldBlob,
                         const uint64_t *oldOffsets, const uint8_t *blob, size_t blobCap, const uint64_t *offsets, const int32_t *tileIndices,
                         const int32_t *status, bool onDevice, GfBlockGeom &g, GfBlockCutElem *cut)
{
    if (!grid || !rect || !status) return GF_ERR_ARG;
    const gf_status sg = blockGeom(grid, rect, g);
    if (sg == GF_ERR_ARG) return sg;
    const size_t nOut = sg == GF_OK ? (size_t)g.nTileRows * (size_t)g.nTileCols : 1;
    const gf_status se = encArgs(c, codecs, nCodecs, elems, nElems, grid->n_rows_tile, grid->n_cols_tile, nOut, tileIndices, blocks, blob, blobCap,
                                 offsets, onDevice, status);
    if (se == GF_ERR_ARG) return se;
    gf_status so = GF_OK;
    if (nOld)
        so = elemsArgs(c, codecs, nCodecs, elems, nElems, grid->n_rows_tile, grid->n_cols_tile, nOld, oldBlob, onDevice, oldOffsets,
                       const_cast<void *const *>(blocks), status);
    if (so == GF_ERR_ARG) return so;
    if (cutElems(elems, ranges, nElems, cut) != GF_OK) return GF_ERR_ARG;
    return firstOf(sg, firstOf(se, so));
}

namespace {

// the layout of the small per-tile results in dBwMeta: flags | pre-status
struct BwMeta {
    Carve k;
    size_t flags, pre;
    explicit BwMeta(size_t nOut) : flags(k.add(nOut * 4)), pre(k.add(nOut * 4)) {}
};

// blocks in device memory -> cut tiles in dBwTiles (dTiles[e]), pre-status in dBwMeta, tile indices in dTileIndices (the caller holds
// the lock and has checked the arguments).  With old records it synchronises the stream once (the records driver does).
gf_status blockCutDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const GfBlockGeom &g,
                      const GfBlockCutElem *cut, const void *const *dBlocks, size_t nOld, const uint8_t *dOldBlob, size_t oldBytes,
                      const uint64_t *dOldOffsets, int verifyOld, int32_t *dTileIndices, const void **dTiles, const uint64_t *dOldEnds = nullptr)
{
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = streamOf(c, stream);
    const size_t cells = (size_t)g.nRowsTile * (size_t)g.nColsTile, nOut = (size_t)g.nTileRows * (size_t)g.nTileCols;
    const BwMeta m(nOut);
    // the cut tiles: n_elems arrays of n_out * cells items with room behind a SHORT array's last word; the old records' tiles
    void *cutTiles[GF_MAX_ELEMS], *dOld[GF_MAX_ELEMS];
    gf_status s;
    if ((s = elemArrays(c->dBwTiles, elems, nElems, nOut * cells, cutTiles, 4)) != GF_OK) return s;
    if ((s = c->dBwMeta.ensure(m.k)) != GF_OK) return s;
    uint8_t *meta = (uint8_t *)c->dBwMeta.p;
    GfBlockCutElemsArgs q{};
    q.nElems = nElems;
    q.flags = (uint32_t *)(meta + m.flags);
    q.g = g;
    for (int e = 0; e < nElems; e++) {
        q.elems[e] = cut[e];
        q.elems[e].block = dBlocks[e];
        q.elems[e].tiles = cutTiles[e];
        dTiles[e] = cutTiles[e];
    }
    GfBlockWriteVerdictArgs v{};
    if (nOld) {
        // the old records, decoded into the block read's temporaries; an ICF element as INT: its codes come back, not floats
        Carve idx;
        const size_t idxAt = idx.add(nOld * 4), statusAt = idx.add((size_t)nElems * nOld * 4);
        if ((s = elemArrays(c->dBlockTmp, elems, nElems, nOld * cells, dOld)) != GF_OK) return s;
        if ((s = c->dBlockIdx.ensure(idx)) != GF_OK) return s;
        if ((s = c->dBlockSlots.ensure(nOut * 4 + 16)) != GF_OK) return s;
        int32_t *dOldIdx = c->dBlockIdx.at<int32_t>(idxAt), *dOldStatus = c->dBlockIdx.at<int32_t>(statusAt);
        gf_elem_spec asInt[GF_MAX_ELEMS];
        for (int e = 0; e < nElems; e++) {
            asInt[e] = elems[e];
            if (asInt[e].type == GF_ELEM_ICF) asInt[e].type = GF_ELEM_INT;
            q.elems[e].oldTiles = dOld[e];
        }
        GF_HIP(hipMemsetAsync(dOldIdx, 0xff, nOld * 4, st));                    // (the driver leaves a failed record's entry alone: -1 places nothing)
        s = recordsDecodeDev(c, stream, codecs, nCodecs, asInt, nElems, g.nRowsTile, g.nColsTile, nOld, dOldBlob, oldBytes, dOldOffsets, nullptr,
                             verifyOld, dOldIdx, dOld, dOldStatus, dOldEnds);
        if (s != GF_OK) return s;
        GF_HIP(hipMemsetAsync(c->dBlockSlots.p, 0xff, nOut * 4, st));
        GfBlockSlotsArgs p{};
        p.tileIndices = dOldIdx;
        p.nRecords = nOld;
        p.slots = (int32_t *)c->dBlockSlots.p;
        p.g = g;
        GF_HIP(gf_launch_block_slots(p, st));
        q.slots = v.slots = p.slots;
        v.oldStatus = dOldStatus;
        v.nOld = nOld;
    }
    GF_HIP(hipMemsetAsync(q.flags, 0, nOut * 4, st));
    GF_HIP(gf_launch_block_cut_elems(q, st));
    v.flags = q.flags;
    v.nElems = nElems;
    v.preStatus = (int32_t *)(meta + m.pre);
    v.tileIndices = dTileIndices;
    v.g = g;
    GF_HIP(gf_launch_block_write_verdict(v, st));
    return GF_OK;
}

}  // namespace

// blocks in device memory -> records in device memory: the cut, then the record writer with the cut's verdict as its pre-status (no
// lock taken, no argument checked: its callers hold the context's lock).  dOldEnds (may be null): an explicit end per old record, as the
// records driver takes it: the old records of a file image, where they lie (gvrs_api_file_update.hip)
gf_status blockWriteDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const GfBlockGeom &g,
                        const GfBlockCutElem *cut, const void *const *dBlocks, size_t nOld, const uint8_t *dOldBlob, size_t oldBlobBytes,
                        const uint64_t *dOldOffsets, int verifyOldChecksum, int checksumEnabled, uint8_t *dBlob, size_t blobCap, uint64_t *dOffsets,
                        int32_t *dTileIndices, uint8_t *dCodecUsed, int32_t *dStatus, const uint64_t *dOldEnds)
{
    const void *dTiles[GF_MAX_ELEMS];
    const gf_status s = blockCutDev(c, stream, codecs, nCodecs, elems, nElems, g, cut, dBlocks, nOld, dOldBlob, oldBlobBytes, dOldOffsets,
                                    verifyOldChecksum, dTileIndices, dTiles, dOldEnds);
    if (s != GF_OK) return s;
    const size_t nOut = (size_t)g.nTileRows * (size_t)g.nTileCols;
    const BwMeta m(nOut);
    return recordsEncodeDev(c, stream, codecs, nCodecs, elems, nElems, g.nRowsTile, g.nColsTile, nOut, dTileIndices, dTiles, checksumEnabled, dBlob,
                            blobCap, dOffsets, dCodecUsed, dStatus, (const int32_t *)((uint8_t *)c->dBwMeta.p + m.pre));
}

// the tail of a host form that writes records (gvrs_api_internal.h); gf_block_write_elems and gf_file_update_points_elems end in it
gf_status hostWriteTail(gf_context *c, HostStage &sg, const HostWriteParts &p, bool onDevice, const int *codecs, int nCodecs, const gf_elem_spec *elems,
                        int nElems, int nRowsTile, int nColsTile, size_t nOut, const void *const *dTiles, const int32_t *dPre, int checksumEnabled,
                        size_t maxBlob, uint8_t *blob, size_t blobCap, uint64_t *offsets, int32_t *tileIndices, uint8_t *codecUsed, int32_t *status)
{
    const size_t cells = (size_t)nRowsTile * (size_t)nColsTile, nInst = (size_t)nElems * nOut;
    gf_status s;
    if (onDevice) {
        s = recordsEncodeDev(c, c->stream, codecs, nCodecs, elems, nElems, nRowsTile, nColsTile, nOut, sg.ptr<int32_t>(p.indices), dTiles,
                             checksumEnabled, sg.ptr<uint8_t>(p.blob), maxBlob, sg.ptr<uint64_t>(p.offsets), sg.ptr<uint8_t>(p.used),
                             sg.ptr<int32_t>(p.status), dPre);
        if (s != GF_OK || (s = sg.flush()) != GF_OK) return s;
        gf_status first = GF_OK;
        for (size_t t = 0; t < nOut && first == GF_OK; t++)
            if (status[t] < 0) first = (gf_status)status[t];
        if (offsets[nOut] > blobCap) return first != GF_OK ? first : GF_ERR_CAPACITY;
        if (offsets[nOut] && ((s = sg.fetch(p.blob, (size_t)offsets[nOut])) != GF_OK || (s = sg.end()) != GF_OK)) return s;
        return first;
    }
    // a list that needs the host's zlib: the cut tiles and the verdicts come back from the device form's temporaries, the tiles that
    // get a record go through the host encoders (which stage for themselves: this call's stage ends first), and the records are
    // laid out with zero-length records for the others
    std::vector<std::vector<uint8_t>> tiles(nElems);
    for (int e = 0; e < nElems; e++) {
        const size_t tb = nOut * cells * elemItemBytes(elems[e].type);
        tiles[e].resize(tb + 4);                                                // (4 spare bytes: readable to the end of a SHORT array's last word)
        GF_HIP(hipMemcpyAsync(tiles[e].data(), dTiles[e], tb, hipMemcpyDeviceToHost, c->stream));
    }
    GF_HIP(hipMemcpyAsync(status, dPre, nOut * 4, hipMemcpyDeviceToHost, c->stream));
    if ((s = sg.end()) != GF_OK) return s;
    std::vector<size_t> keep;
    gf_status first = GF_OK;
    for (size_t t = 0; t < nOut; t++) {
        if (status[t] == GF_OK) keep.push_back(t);
        else if (status[t] < 0 && first == GF_OK) first = (gf_status)status[t];
    }
    const size_t nKeep = keep.size();
    std::vector<int32_t> keptIdx(nKeep);
    const void *keptValues[GF_MAX_ELEMS];
    for (int e = 0; e < nElems; e++) {                                          // (compacted in place: keep[k] >= k)
        const size_t tb = cells * elemItemBytes(elems[e].type);
        for (size_t k = 0; k < nKeep; k++)
            if (keep[k] != k) memmove(tiles[e].data() + k * tb, tiles[e].data() + keep[k] * tb, tb);
        tiles[e].resize(nKeep * tb + 4);                                        // (never grows: sized with the spare bytes above)
        keptValues[e] = tiles[e].data();
    }
    for (size_t k = 0; k < nKeep; k++) keptIdx[k] = tileIndices[keep[k]];
    std::vector<uint64_t> keptOff(nKeep + 1, 0);
    std::vector<uint8_t> keptUsed(nInst ? (size_t)nElems * nKeep + 1 : 1);
    if (nKeep) {
        s = recordsEncodeHost(c, codecs, nCodecs, elems, nElems, nRowsTile, nColsTile, nKeep, keptIdx.data(), keptValues, checksumEnabled, blob,
                              blobCap, keptOff.data(), keptUsed.data());
        if (s != GF_OK && s != GF_ERR_CAPACITY) return s;
    } else s = GF_OK;
    if (codecUsed) memset(codecUsed, 0xff, nInst);
    size_t k = 0;
    for (size_t t = 0; t < nOut; t++) {
        offsets[t] = keptOff[k];
        if (k < nKeep && keep[k] == t) {
            if (codecUsed)
                for (int e = 0; e < nElems; e++) codecUsed[(size_t)e * nOut + t] = keptUsed[(size_t)e * nKeep + k];
            k++;
        }
    }
    offsets[nOut] = keptOff[nKeep];
    return first != GF_OK ? first : s;
}

extern "C" {

gf_status gf_block_tile_rect(const gf_grid_spec *grid, const gf_rect *rect, int32_t *tileRow0, int32_t *tileCol0, int32_t *nTileRows,
                             int32_t *nTileCols)
{
    if (!tileRow0 || !tileCol0 || !nTileRows || !nTileCols) return GF_ERR_ARG;
    GfBlockGeom g{};
    const gf_status s = blockGeom(grid, rect, g);
    if (s != GF_OK) return s;
    *tileRow0 = g.tileRow0, *tileCol0 = g.tileCol0, *nTileRows = g.nTileRows, *nTileCols = g.nTileCols;
    return GF_OK;
}

gf_status gf_block_write_elems_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems,
                                   const gf_elem_range *ranges, int nElems, const gf_grid_spec *grid, const gf_rect *rect,
                                   const void *const *dBlocks, size_t nOld, const uint8_t *dOldBlob, size_t oldBlobBytes,
                                   const uint64_t *dOldOffsets, int verifyOldChecksum, int checksumEnabled, uint8_t *dBlob, size_t blobCap,
                                   uint64_t *dOffsets, int32_t *dTileIndices, uint8_t *dCodecUsed, int32_t *dStatus)
{
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    gf_status s = blockWriteArgs(c, codecs, nCodecs, elems, ranges, nElems, grid, rect, dBlocks, nOld, dOldBlob, dOldOffsets, dBlob, blobCap, dOffsets,
                                 dTileIndices, dStatus, true, g, cut);
    if (s != GF_OK) return s;
    if (!deviceList(codecs, nCodecs, elems, nElems)) return GF_ERR_UNSUPPORTED;
    GF_CTX_LOCK(c);
    return blockWriteDev(c, stream, codecs, nCodecs, elems, nElems, g, cut, dBlocks, nOld, dOldBlob, oldBlobBytes, dOldOffsets, verifyOldChecksum,
                         checksumEnabled, dBlob, blobCap, dOffsets, dTileIndices, dCodecUsed, dStatus);
}

#ifdef GF_DIAG
// The diagnostic flavour of the library only, for tools/block_write_rate.py (loaded by name; not part of include/gvrs_hip_codec.h):
// the first stage of gf_block_write_elems_dev alone, without old records -- the flags' memset, k_block_cut_elems and
// k_block_write_verdict.  The cut tiles stay in the context.  The shipping library has one way into blockCutDev.
gf_status gf_internal_block_cut_elems_dev(gf_context *c, void *stream, const gf_elem_spec *elems, const gf_elem_range *ranges, int nElems,
                                          const gf_grid_spec *grid, const gf_rect *rect, const void *const *dBlocks, int32_t *dTileIndices)
{
    if (!c || !elems || !dBlocks || !dTileIndices || nElems < 1 || nElems > GF_MAX_ELEMS) return GF_ERR_ARG;
    for (int e = 0; e < nElems; e++)
        if (!dBlocks[e] || elems[e].type < GF_ELEM_INT || elems[e].type > GF_ELEM_ICF) return GF_ERR_ARG;
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    gf_status s = blockGeom(grid, rect, g);
    if (s != GF_OK) return s;
    if (cutElems(elems, ranges, nElems, cut) != GF_OK) return GF_ERR_ARG;
    GF_CTX_LOCK(c);
    const void *dTiles[GF_MAX_ELEMS];
    return blockCutDev(c, stream, nullptr, 0, elems, nElems, g, cut, dBlocks, 0, nullptr, 0, nullptr, 0, dTileIndices, dTiles);
}
#endif

gf_status gf_block_write_elems(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, const gf_elem_range *ranges, int nElems,
                               const gf_grid_spec *grid, const gf_rect *rect, const void *const *blocks, size_t nOld, const uint8_t *oldBlob,
                               const uint64_t *oldOffsets, int verifyOldChecksum, int checksumEnabled, uint8_t *blob, size_t blobCap,
                               uint64_t *offsets, int32_t *tileIndices, uint8_t *codecUsed, int32_t *status)
{
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    gf_status s = blockWriteArgs(c, codecs, nCodecs, elems, ranges, nElems, grid, rect, blocks, nOld, oldBlob, oldOffsets, blob, blobCap, offsets,
                                 tileIndices, status, false, g, cut);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    if (nCodecs < 0) nCodecs = 0;
    const bool onDevice = deviceList(codecs, nCodecs, elems, nElems);
    const size_t nOut = (size_t)g.nTileRows * (size_t)g.nTileCols;
    const size_t blockCells = (size_t)g.nRows * (size_t)g.nCols, oldBytes = nOld ? (size_t)oldOffsets[nOld] : 0;
    const size_t nInst = (size_t)nElems * nOut;
    const size_t maxBlob = onDevice ? nOut * gf_tile_record_max_bytes_elems(elems, nElems, g.nRowsTile, g.nColsTile) : 0;
    // staging: the block of element 0, 1, ... | old blob | old offsets | tile indices, and for a device list the records at their
    // largest | offsets | statuses | codec used; the offsets say how much of the records counts
    HostStage sg(c);
    int blockP[GF_MAX_ELEMS];
    stageElems(sg, STAGE_IN, elems, nElems, blockCells, blocks, blockP);
    const int oldP = sg.in(nOld ? oldBlob : nullptr, oldBytes, 32), oldOffP = sg.in(nOld ? oldOffsets : nullptr, (nOld + 1) * 8);
    const int indicesP = sg.out(tileIndices, nOut * 4);
    const int blobP = sg.held(blob, maxBlob), offsetsP = sg.out(onDevice ? offsets : nullptr, (nOut + 1) * 8);
    const int statusP = sg.out(onDevice ? status : nullptr, nOut * 4), usedP = sg.out(onDevice ? codecUsed : nullptr, nInst);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dBlocks[GF_MAX_ELEMS];
    sg.ptrs(blockP, nElems, dBlocks);
    const BwMeta m(nOut);
    if ((s = c->dBwMeta.ensure(m.k)) != GF_OK) return s;                       // (before its address is taken: blockCutDev asks for no more)
    const int32_t *dPre = c->dBwMeta.at<int32_t>(m.pre);
    const void *dTiles[GF_MAX_ELEMS];
    s = blockCutDev(c, c->stream, codecs, nCodecs, elems, nElems, g, cut, dBlocks, nOld, sg.ptr<uint8_t>(oldP), oldBytes, sg.ptr<uint64_t>(oldOffP),
                    verifyOldChecksum, sg.ptr<int32_t>(indicesP), dTiles);
    if (s != GF_OK) return s;
    return hostWriteTail(c, sg, HostWriteParts{indicesP, blobP, offsetsP, statusP, usedP}, onDevice, codecs, nCodecs, elems, nElems, g.nRowsTile,
                         g.nColsTile, nOut, dTiles, dPre, checksumEnabled, maxBlob, blob, blobCap, offsets, tileIndices, codecUsed, status);
}

}  // extern "C"
