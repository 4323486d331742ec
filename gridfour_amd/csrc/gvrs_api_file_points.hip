// gvrs_api_file_points.hip -- GVRS files read at scattered POINTS: cells (GvrsElement.readValue / readValueInt over a batch) and
// B-spline interpolation (GvrsInterpolatorBSpline.z / zNormal over a batch) straight from a file image, decoding only the tiles
// the points touch.  gf_file_cells_tiles / gf_file_interp_tiles are host arithmetic (gvrs_file_points.h; no device, no context).
// The device forms mark and rank the touched tiles (k_points_mark, k_points_rank), learn their count (the first synchronisation),
// locate their records in the image (k_file_locate over the list), decode them into a pool through the records' pipeline of
// gvrs_api_records_dev.hip (the second synchronisation) and sample the pool (k_points_cells, k_points_interp).  The host forms
// take the touched tiles from the two host functions, look their records up in the host image and stage them end to end, as
// gf_file_read_block_elems does; the tail behind the lookup is one function for both.
// And WRITTEN at scattered points (GvrsElement.writeValue / writeValueInt over a batch into a file opened "rw", then close()):
// gf_file_update_points_elems[_dev] mark, rank and locate the touched tiles as the reads do, judge the old records' heads as an
// update does (k_points_heads; the host form on the host), decode them into the pool, store the points' values into it by the
// cell rule of gvrs_file_points_store.h (k_points_prepare, k_points_claim, k_points_store, k_points_verdict:
// gvrs_file_points_write.hip; pointsWriteCells is that stretch for both forms), write the touched tiles' records from the pool
// (the record writer of gvrs_api_records_enc.hip with the verdict as its pre-status; the host form through hostWriteTail, which
// takes any codec list) and place them in ascending tile index (updateRecordsDev of gvrs_api_file_update.hip; the host form
// through gfFileUpdateAssemble).
// Reference: gvrs/TileAccessIndices.java:78-92, gvrs/GvrsElement.java (readValue), gvrs/GvrsInterpolatorBSpline.java:283-334, :374-484,
// gvrs/TileElement{Int,Short,Float,IntCodedFloat}.java (setValue), gvrs/RasterTileCache.java, gvrs/RecordManager.java:386-490.

#include "gvrs_api_internal.h"
#include "gvrs_file_update.h"

namespace {

constexpr int64_t POINTS_MAX_TILES_GRID = (int64_t)1 << 27;                    // bitmap and prefixes: 16 MB each at the most

GfPointsGrid gridOf(const gf_file_info &i) { return gf_points_grid(i.grid.n_rows_grid, i.grid.n_cols_grid, i.grid.n_rows_tile, i.grid.n_cols_tile); }

// ---- the touched tiles on the host: the bitmap the kernels build, built by the same functions ----
void setBit(std::vector<uint32_t> &bits, int32_t tile) { bits[(uint32_t)tile >> 5] |= 1u << ((uint32_t)tile & 31u); }

std::vector<uint32_t> cellsBits(const GfPointsGrid &g, size_t n, const int32_t *rows, const int32_t *cols)
{
    std::vector<uint32_t> bits(gf_points_words(g.nTilesGrid), 0u);
    for (size_t t = 0; t < n; t++) {
        int32_t tile, at;
        if (gf_points_cell(g, rows[t], cols[t], tile, at)) setBit(bits, tile);
    }
    return bits;
}

std::vector<uint32_t> windowsBits(const GfPointsGrid &g, const GfInterpGeom &ig, size_t n, const double *rows, const double *cols)
{
    std::vector<uint32_t> bits(gf_points_words(g.nTilesGrid), 0u);
    for (size_t t = 0; t < n; t++) {
        GfInterpWindow w;
        if (gf_interp_window(ig, rows[t], cols[t], w) != GF_IP_OK) continue;
        const GfWindowTiles wt = gf_points_window_tiles(g, w.row0, w.col0, w.n1);
        for (int32_t k = 0, nk = wt.count(); k < nk; k++) setBit(bits, wt.at(k));
    }
    return bits;
}

// ... of points given as kind says (gf_coords_query, the function the kernels call): a refused point touches no tile
std::vector<uint32_t> coordsBits(const GfPointsGrid &g, const GfInterpGeom &ig, const GfCoords &co, int kind, size_t n, const double *a, const double *b)
{
    std::vector<uint32_t> bits(gf_points_words(g.nTilesGrid), 0u);
    for (size_t t = 0; t < n; t++) {
        GfCoordsQuery q;
        GfInterpWindow w;
        if (gf_coords_query(co, kind, a[t], b[t], 0.0, false, q) != GF_IP_OK || gf_interp_window(ig, q.row, q.col, w) != GF_IP_OK) continue;
        const GfWindowTiles wt = gf_points_window_tiles(g, w.row0, w.col0, w.n1);
        for (int32_t k = 0, nk = wt.count(); k < nk; k++) setBit(bits, wt.at(k));
    }
    return bits;
}

// the bitmap's tiles in ascending order: at most cap of them into tiles, all of them counted
size_t listBits(const std::vector<uint32_t> &bits, int32_t *tiles, size_t cap)
{
    size_t n = 0;
    for (size_t w = 0; w < bits.size(); w++)
        for (uint32_t word = bits[w]; word != 0u; word &= word - 1u, n++)
            if (n < cap) tiles[n] = (int32_t)(w * 32u + (uint32_t)__builtin_ctz(word));
    return n;
}

// ---- argument checks (before the context or a device is looked at) ----
// what the interpolation forms read of a spec; fills ig for the whole grid of the file and element elem (elem < 0: no element)
gf_status pointsSpecArgs(const gf_file_info &i, const gf_interp_spec *spec, int elem, bool perPointSpacing, GfInterpGeom &ig)
{
    if (!spec) return GF_ERR_ARG;
    if (i.grid.n_rows_grid < 4 || i.grid.n_cols_grid < 4) return GF_ERR_ARG;                       // (GvrsInterpolatorBSpline.java:113-116)
    if (spec->wrap < 0 || spec->wrap > 2 || spec->target < GF_INTERP_VALUE || spec->target > GF_INTERP_SECOND) return GF_ERR_ARG;
    if (elem >= i.n_elems) return GF_ERR_ARG;
    if (elem >= 0 && spec->target >= GF_INTERP_FIRST && (spec->row_spacing == 0 || (spec->col_spacing == 0 && !perPointSpacing))) return GF_ERR_ARG;
    ig = GfInterpGeom{};
    gf_points_whole_grid(ig, gridOf(i));
    ig.elemType = elem >= 0 ? i.elems[elem].type : GF_ELEM_INT, ig.fillI = elem >= 0 ? i.elems[elem].fill_i : 0;
    ig.wrap = spec->wrap, ig.target = spec->target;
    ig.rowSpacing = spec->row_spacing, ig.colSpacing = spec->col_spacing;
    ig.rowFringe0 = spec->row_fringe0, ig.rowFringe1 = spec->row_fringe1, ig.colFringe0 = spec->col_fringe0, ig.colFringe1 = spec->col_fringe1;
    return GF_OK;
}

// what all four reads check of file, image and counts; fills the codec list and the fills' bits as the records' calls take them
gf_status pointsFileArgs(const gf_context *c, const gf_file_info &i, const uint8_t *image, size_t imageBytes, bool onDevice, size_t nPoints,
                         size_t maxTiles, int *codecs, uint32_t *fill)
{
    if (!c || !image) return GF_ERR_ARG;
    if (onDevice && ((uintptr_t)image & 7) != 0) return GF_ERR_ARG;
    if (imageBytes < i.content_pos) return GF_ERR_ARG;                            // (not the image that was opened)
    for (int k = 0; k < i.n_codecs; k++) codecs[k] = i.codecs[k] == GF_CODEC_UNKNOWN ? GF_CODEC_NONE : i.codecs[k];
    // (values, offsets and statuses of the records' checks: their places are taken by the image, which is only looked at for null)
    const void *some[GF_MAX_ELEMS];
    for (int e = 0; e < GF_MAX_ELEMS; e++) some[e] = image;
    const gf_status sa = elemsArgs(c, codecs, i.n_codecs, i.elems, i.n_elems, i.grid.n_rows_tile, i.grid.n_cols_tile, 0, image, onDevice,
                                   (const uint64_t *)image, (void *const *)some, (const int32_t *)image);
    const gf_status s = firstOf(sa, elemFills(i.elems, i.n_elems, fill));
    if (s != GF_OK) return s;
    for (int k = 0; k < i.n_codecs; k++)
        if (i.codecs[k] == GF_CODEC_UNKNOWN) return GF_ERR_UNSUPPORTED;
    if (gfTilesOfGrid(i.grid).count() > POINTS_MAX_TILES_GRID) return GF_ERR_UNSUPPORTED;
    if (nPoints > 0x7fffffffull || maxTiles > 0x7fffffffull / (size_t)i.n_elems) return GF_ERR_UNSUPPORTED;   // (they travel as 32 bits)
    return GF_OK;
}

// the answer of the forms at coordinates to a NULL context: what can be judged of the image without one comes first
gf_status pointsNoContext(const gf_file_info &i, const uint8_t *image, size_t imageBytes, bool onDevice)
{
    if ((onDevice && ((uintptr_t)image & 7) != 0) || imageBytes < i.content_pos) return GF_ERR_ARG;
    return noContext();
}

gf_status interpOutArgs(const gf_interp_spec *spec, const gf_interp_out *out)
{
    if (!spec || !out || !out->z) return GF_ERR_ARG;
    if (spec->target == GF_INTERP_VALUE && out->normal) return GF_ERR_ARG;
    return GF_OK;
}

// ---- the device side ----
// the context's part of a call, sized by maxTiles before the first launch (the count is learnt behind it, and a buffer that grew
// would have moved): bitmap | prefixes | count || list | starts | ends | verdicts | the records' tile indices | slot statuses
struct PointsBuf {
    uint32_t *bits, *prefix, *count;
    int32_t *list, *verdict, *indices, *slotStatus;
    uint64_t *starts, *ends;
    size_t nWords;
};
gf_status pointsBuf(gf_context *c, const GfPointsGrid &g, int nElems, size_t maxTiles, bool withExtents, PointsBuf &b)
{
    Carve k;
    b.nWords = gf_points_words(g.nTilesGrid);
    const size_t bitsAt = k.add(b.nWords * 4), prefixAt = k.add(b.nWords * 4), countAt = k.add(16), listAt = k.add(maxTiles * 4);
    const size_t startsAt = k.add(withExtents ? maxTiles * 8 : 0), endsAt = k.add(withExtents ? maxTiles * 8 : 0);
    const size_t verdictAt = k.add(withExtents ? maxTiles * 4 : 0), indicesAt = k.add(maxTiles * 4), statusAt = k.add((size_t)nElems * maxTiles * 4);
    const gf_status s = c->dFilePoints.ensure(k);
    if (s != GF_OK) return s;
    const DevBuf &B = c->dFilePoints;
    b.bits = B.at<uint32_t>(bitsAt), b.prefix = B.at<uint32_t>(prefixAt), b.count = B.at<uint32_t>(countAt);
    b.list = B.at<int32_t>(listAt), b.starts = B.at<uint64_t>(startsAt), b.ends = B.at<uint64_t>(endsAt);
    b.verdict = B.at<int32_t>(verdictAt), b.indices = B.at<int32_t>(indicesAt), b.slotStatus = B.at<int32_t>(statusAt);
    return GF_OK;
}

// what a call samples: cells of every element, or the windows of one
struct PointsWhat {
    bool windows;
    size_t nPoints;
    const int32_t *rowsI, *colsI;                 // cells (device)
    void *const *values;                          // HOST array of device pointers
    int32_t *status;
    GfInterpGeom ig;                              // windows
    int elem;
    const double *rowsD, *colsD, *colSpacing;
    GfInterpArgs out;                             // its output pointers alone
    bool coords;                                  // windows of points given as kind says: rowsD / colsD are their a / b
    int kind;
    GfCoords co;
    double *spacingUsed;                          // may be null
};

// bitmap zeroed, k_points_mark, k_points_rank (enqueued)
gf_status pointsMarkRank(hipStream_t st, const GfPointsGrid &g, const PointsWhat &w, const PointsBuf &b, size_t maxTiles)
{
    GF_HIP(hipMemsetAsync(b.bits, 0, b.nWords * 4, st));
    GfPointsMarkArgs m{};
    m.g = g, m.ig = w.ig, m.nPoints = w.nPoints;
    m.rowsI = w.rowsI, m.colsI = w.colsI, m.rowsD = w.rowsD, m.colsD = w.colsD;
    m.bits = b.bits;
    if (w.coords) GF_HIP(gf_launch_points_mark_coords(GfPointsMarkCoordsArgs{m, w.co, w.kind}, st));
    else GF_HIP(gf_launch_points_mark(m, w.windows, st));
    GfPointsRankArgs r{};
    r.bits = b.bits, r.nWords = (uint32_t)b.nWords, r.prefix = b.prefix, r.list = b.list, r.maxTiles = (uint32_t)maxTiles, r.count = b.count;
    GF_HIP(gf_launch_points_rank(r, st));
    return GF_OK;
}

// THE TAIL both forms share: the n touched tiles' records -- slot s = [dStarts[s], dEnds[s]) of dBlob, the empty extent where
// dVerdict[s] is not GF_FILE_LOCATED -- decoded into the pool (n * cells items per element, in dBlockTmp: one stream at a time,
// as the block reads), the verdicts put into the slots' statuses, the pool sampled.  No lock taken, no argument checked.
gf_status pointsTail(gf_context *c, hipStream_t st, const gf_file_info &i, const GfPointsGrid &g, const int *codecs, const uint32_t *fill, size_t n,
                     const uint8_t *dBlob, size_t blobBytes, const uint64_t *dStarts, const uint64_t *dEnds, const int32_t *dVerdict,
                     int verifyChecksum, const PointsBuf &b, const PointsWhat &w)
{
    const size_t cells = (size_t)g.nRowsTile * (size_t)g.nColsTile;
    void *dPool[GF_MAX_ELEMS];
    gf_status s;
    if ((s = elemArrays(c->dBlockTmp, i.elems, i.n_elems, n * cells, dPool)) != GF_OK) return s;
    if (n) {
        s = recordsDecodeDev(c, st, codecs, i.n_codecs, i.elems, i.n_elems, g.nRowsTile, g.nColsTile, n, dBlob, blobBytes, dStarts, nullptr,
                             verifyChecksum, b.indices, dPool, b.slotStatus, dEnds);
        if (s != GF_OK) return s;
        GF_HIP(gf_launch_file_status(dVerdict, b.slotStatus, n, i.n_elems, st));
    }
    GfPointsLookup look{b.bits, b.prefix, dVerdict, b.slotStatus, (uint32_t)n, (uint32_t)cells};
    if (!w.windows) {
        GfPointsCellsArgs a{};
        a.g = g, a.look = look, a.nPoints = w.nPoints, a.rows = w.rowsI, a.cols = w.colsI, a.status = w.status, a.nElems = i.n_elems;
        for (int e = 0; e < i.n_elems; e++) a.elems[e] = GfPointsElem{dPool[e], w.values[e], fill[e], (uint32_t)elemItemBytes(i.elems[e].type)};
        GF_HIP(gf_launch_points_cells(a, st));
    } else {
        GfPointsInterpArgs a{};
        a.g = g, a.ig = w.ig, a.look = look;
        a.look.slotStatus = b.slotStatus + (size_t)w.elem * n;
        a.pool = dPool[w.elem], a.fillBits = fill[w.elem];
        a.nPoints = w.nPoints, a.rows = w.rowsD, a.cols = w.colsD, a.colSpacing = w.colSpacing;
        a.z = w.out.z, a.zx = w.out.zx, a.zy = w.out.zy, a.zxx = w.out.zxx, a.zxy = w.out.zxy, a.zyy = w.out.zyy;
        a.normal = w.out.normal, a.status = w.out.status;
        if (w.coords) GF_HIP(gf_launch_points_interp_coords(GfPointsInterpCoordsArgs{a, w.co, w.kind, w.spacingUsed}, st));
        else GF_HIP(gf_launch_points_interp(a, st));
    }
    return GF_OK;
}

// the device forms behind their checks: mark, rank, the count (synchronises), locate over the list, the tail
gf_status pointsDev(gf_context *c, const gf_file_info &i, const uint8_t *dImage, size_t imageBytes, const int *codecs, const uint32_t *fill,
                    int verifyChecksum, size_t maxTiles, const PointsWhat &w, size_t *nTouched)
{
    *nTouched = 0;
    if (w.nPoints == 0) return GF_OK;
    if (!i.checksum_enabled) verifyChecksum = 0;                                  // (the records of such a file carry none)
    const GfPointsGrid g = gridOf(i);
    if (maxTiles > (size_t)g.nTilesGrid) maxTiles = (size_t)g.nTilesGrid;         // (no set of points touches more)
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    PointsBuf b;
    gf_status s;
    if ((s = pointsBuf(c, g, i.n_elems, maxTiles, true, b)) != GF_OK) return s;
    if ((s = c->hRecCounts.ensure(256 * 4)) != GF_OK) return s;
    if ((s = pointsMarkRank(st, g, w, b, maxTiles)) != GF_OK) return s;
    // the first synchronisation: the host sizes the pool and the records' pipeline by the count
    GF_HIP(hipMemcpyAsync(c->hRecCounts.p, b.count, 4, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    const size_t n = *(const uint32_t *)c->hRecCounts.p;
    *nTouched = n;
    if (n > maxTiles) return GF_ERR_CAPACITY;                                     // (nothing of the outputs has been written)
    GfFileLocateArgs a{};
    a.image = dImage, a.imageBytes = imageBytes, a.dir = gfFileDirOf(i);
    a.starts = b.starts, a.ends = b.ends, a.verdict = b.verdict;
    a.tileList = b.list, a.nList = (uint32_t)n;
    GF_HIP(gf_launch_file_locate(a, st));
    return pointsTail(c, st, i, g, codecs, fill, n, dImage, imageBytes, b.starts, b.ends, b.verdict, verifyChecksum, b, w);
}

// The host forms behind their checks.  The touched tiles (bits: the host's bitmap) are looked up in the host image; a record the
// framing walk would refuse for its size word is refused here, so that the staged records are whole, multiples of 8 and end to
// end (as gf_file_read_block_elems).  stage(sg, w) declares the call's coordinates and outputs and fills w with their places.
template <class Declare, class Place>
gf_status pointsHost(gf_context *c, const gf_file_info &i, const uint8_t *image, size_t imageBytes, const int *codecs, const uint32_t *fill,
                     int verifyChecksum, size_t maxTiles, const std::vector<uint32_t> &bits, PointsWhat &w, size_t *nTouched, Declare declare,
                     Place place)
{
    *nTouched = 0;
    if (w.nPoints == 0) return GF_OK;
    if (!i.checksum_enabled) verifyChecksum = 0;
    const GfPointsGrid g = gridOf(i);
    const size_t n = listBits(bits, nullptr, 0);
    *nTouched = n;
    if (n > maxTiles) return GF_ERR_CAPACITY;
    std::vector<int32_t> list(n), verdict(n);
    listBits(bits, list.data(), n);
    std::vector<uint64_t> from, starts(n, 0), ends(n, 0);
    uint64_t blobBytes = 0;
    const GfFileDir dir = gfFileDirOf(i);
    for (size_t s = 0; s < n; s++) {
        uint64_t pos;
        uint32_t size;
        int32_t v = gfFileLocate(dir, image, imageBytes, list[s], &pos, &size);
        if (v == GF_OK && pos != 0) {
            if (size < 20u || (size & 7u) != 0u || (uint64_t)size > imageBytes - (pos - 8)) v = GF_ERR_BOUNDS;
            else {
                v = GF_FILE_LOCATED;
                from.push_back(pos - 8);
                starts[s] = blobBytes, ends[s] = blobBytes + size;
                blobBytes += size;
            }
        }
        verdict[s] = v;
    }
    std::vector<uint8_t> blob((size_t)blobBytes + 16);
    for (size_t s = 0, r = 0; s < n; s++)
        if (verdict[s] == GF_FILE_LOCATED) memcpy(blob.data() + starts[s], image + from[r++], (size_t)(ends[s] - starts[s]));
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    PointsBuf b;
    gf_status s;
    if ((s = pointsBuf(c, g, i.n_elems, n, false, b)) != GF_OK) return s;
    // staging: the records | starts | ends | verdicts | the call's coordinates and outputs
    HostStage sg(c);
    const int blobP = sg.in(blob.data(), (size_t)blobBytes, 32), startsP = sg.in(starts.data(), n * 8), endsP = sg.in(ends.data(), n * 8);
    const int verdictP = sg.in(verdict.data(), n * 4);
    declare(sg);
    if ((s = sg.begin()) != GF_OK) return s;
    place(sg, w);
    // the slots of the tiles on the device come from the device's own bitmap of the staged points (no list, no count read back)
    if ((s = pointsMarkRank(st, g, w, b, 0)) != GF_OK) return s;
    s = pointsTail(c, st, i, g, codecs, fill, n, sg.ptr<uint8_t>(blobP), (size_t)blobBytes, sg.ptr<uint64_t>(startsP), sg.ptr<uint64_t>(endsP),
                   sg.ptr<int32_t>(verdictP), verifyChecksum, b, w);
    return s != GF_OK ? s : sg.end();
}

// ---- writes at points ----
// what both write forms check of handle, image and counts (pointsFileArgs on the handle's file; fills the codec list)
gf_status pointsWriteArgs(const gf_context *c, const GfFileUpdate &h, const uint8_t *image, size_t imageCap, bool onDevice, size_t nPoints, size_t maxTiles,
                          const void *const *values, int *codecs, size_t &maxRecord)
{
    const gf_file_info &i = h.info;
    if (imageCap < h.imageBytes) return GF_ERR_ARG;
    for (int e = 0; e < i.n_elems; e++)
        if (!values[e]) return GF_ERR_ARG;
    uint32_t fill[GF_MAX_ELEMS];
    gf_status s = pointsFileArgs(c, i, image, (size_t)h.imageBytes, onDevice, nPoints, maxTiles, codecs, fill);
    if (s != GF_OK) return s;
    GfBlockGeom g{};
    g.nRowsTile = i.grid.n_rows_tile, g.nColsTile = i.grid.n_cols_tile;
    return fileMaxRecord(i.elems, i.n_elems, g, maxRecord);
}

// THE CELLS of both write forms: the n touched tiles' old records -- slot s = [dStarts[s], dEnds[s]) of dBlob, the empty extent
// where dVerdict[s] is not GF_FILE_LOCATED -- decoded into the pool (dBlockTmp, in the record writer's types: an ICF element as
// INT, its codes), new tiles filled, the points' values stored by the rule "the highest point index whose value passed owns the
// cell" (one owner plane per element in dBwTiles, zeroed here), the points' statuses, the tiles' indices and the pre-status
// (dBwMeta) that the record writer takes.  dList: the touched tiles, ascending.  No lock taken, no argument checked.
gf_status pointsWriteCells(gf_context *c, hipStream_t st, const gf_file_info &i, const GfPointsGrid &g, size_t n, const uint8_t *dBlob,
                           size_t blobBytes, const uint64_t *dStarts, const uint64_t *dEnds, const int32_t *dVerdict, const PointsBuf &b,
                           const int32_t *dList, size_t nPoints, const int32_t *dRows, const int32_t *dCols, const void *const *dValues,
                           int32_t *dPointStatus, int32_t *dTileIndices, void **dPool, const int32_t **dPre)
{
    const size_t cells = (size_t)g.nRowsTile * (size_t)g.nColsTile;
    GfBlockCutElem cut[GF_MAX_ELEMS];
    gf_status s;
    if ((s = cutElems(i.elems, nullptr, i.n_elems, cut)) != GF_OK) return s;
    if ((s = elemArrays(c->dBlockTmp, i.elems, i.n_elems, n * cells, dPool, 4)) != GF_OK) return s;   // (room behind a SHORT array's last word)
    Carve planes, meta;
    size_t planeAt[GF_MAX_ELEMS];
    for (int e = 0; e < i.n_elems; e++) planeAt[e] = planes.add(n * cells * 4);
    const size_t oldAt = meta.add(n * 4), storedAt = meta.add(n * 4), preAt = meta.add(n * 4);
    if ((s = c->dBwTiles.ensure(planes)) != GF_OK || (s = c->dBwMeta.ensure(meta)) != GF_OK) return s;
    if (n) {
        gf_elem_spec asInt[GF_MAX_ELEMS];
        for (int e = 0; e < i.n_elems; e++) {
            asInt[e] = i.elems[e];
            if (asInt[e].type == GF_ELEM_ICF) asInt[e].type = GF_ELEM_INT;
        }
        s = recordsDecodeDev(c, st, i.codecs, i.n_codecs, asInt, i.n_elems, g.nRowsTile, g.nColsTile, n, dBlob, blobBytes, dStarts, nullptr,
                             i.checksum_enabled, b.indices, dPool, b.slotStatus, dEnds);
        if (s != GF_OK) return s;
        GF_HIP(gf_launch_file_status(dVerdict, b.slotStatus, n, i.n_elems, st));
        GF_HIP(hipMemsetAsync(c->dBwTiles.p, 0, planes.total, st));
    }
    GfPointsWriteArgs a{};
    a.g = g;
    a.look = GfPointsLookup{b.bits, b.prefix, dVerdict, b.slotStatus, (uint32_t)n, (uint32_t)cells};
    a.nPoints = nPoints, a.rows = dRows, a.cols = dCols, a.pointStatus = dPointStatus;
    a.list = dList;
    a.slotOld = c->dBwMeta.at<int32_t>(oldAt), a.stored = c->dBwMeta.at<uint32_t>(storedAt);
    a.tileIndices = dTileIndices, a.preStatus = c->dBwMeta.at<int32_t>(preAt);
    a.nElems = i.n_elems;
    for (int e = 0; e < i.n_elems; e++) {
        GfPointsWriteElem &d = a.elems[e];
        d.pool = dPool[e], d.values = dValues[e], d.owner = c->dBwTiles.at<uint32_t>(planeAt[e]);
        d.type = cut[e].type, d.fillBits = cut[e].fillBits, d.fillFBits = cut[e].fillFBits, d.minBits = cut[e].minBits, d.maxBits = cut[e].maxBits;
        d.scale = cut[e].scale, d.offset = cut[e].offset;
    }
    GF_HIP(gf_launch_points_prepare(a, st));
    GF_HIP(gf_launch_points_claim(a, st));
    GF_HIP(gf_launch_points_store(a, st));
    GF_HIP(gf_launch_points_verdict(a, st));
    *dPre = a.preStatus;
    return GF_OK;
}

}  // namespace

extern "C" {

gf_status gf_file_cells_tiles(const gf_file *f, size_t nPoints, const int32_t *rows, const int32_t *cols, int32_t *tiles, size_t tilesCap,
                              size_t *nTiles)
{
    if (!f || !nTiles || (nPoints && (!rows || !cols)) || (tilesCap && !tiles)) return GF_ERR_ARG;
    *nTiles = 0;
    gf_file_info i;
    const gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    if (gfTilesOfGrid(i.grid).count() > POINTS_MAX_TILES_GRID) return GF_ERR_UNSUPPORTED;
    *nTiles = listBits(cellsBits(gridOf(i), nPoints, rows, cols), tiles, tilesCap);
    return GF_OK;
}

gf_status gf_file_interp_tiles(const gf_file *f, const gf_interp_spec *spec, size_t nPoints, const double *rows, const double *cols, int32_t *tiles,
                               size_t tilesCap, size_t *nTiles)
{
    if (!f || !spec || !nTiles || (nPoints && (!rows || !cols)) || (tilesCap && !tiles)) return GF_ERR_ARG;
    *nTiles = 0;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    GfInterpGeom ig;
    if ((s = pointsSpecArgs(i, spec, -1, true, ig)) != GF_OK) return s;
    if (gfTilesOfGrid(i.grid).count() > POINTS_MAX_TILES_GRID) return GF_ERR_UNSUPPORTED;
    *nTiles = listBits(windowsBits(gridOf(i), ig, nPoints, rows, cols), tiles, tilesCap);
    return GF_OK;
}

gf_status gf_file_read_points_elems_dev(gf_context *c, const gf_file *f, const uint8_t *dImage, size_t imageBytes, size_t nPoints,
                                        const int32_t *dRows, const int32_t *dCols, int verifyChecksum, size_t maxTiles, void *const *dValues,
                                        int32_t *dStatus, size_t *nTouched)
{
    if (!c || !f || !dImage || !dValues || !dStatus || !nTouched || (nPoints && (!dRows || !dCols))) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    for (int e = 0; e < i.n_elems; e++)
        if (!dValues[e]) return GF_ERR_ARG;
    int codecs[255];
    uint32_t fill[GF_MAX_ELEMS];
    if ((s = pointsFileArgs(c, i, dImage, imageBytes, true, nPoints, maxTiles, codecs, fill)) != GF_OK) return s;
    PointsWhat w{};
    w.windows = false, w.nPoints = nPoints, w.rowsI = dRows, w.colsI = dCols, w.values = dValues, w.status = dStatus;
    return pointsDev(c, i, dImage, imageBytes, codecs, fill, verifyChecksum, maxTiles, w, nTouched);
}

gf_status gf_file_interp_points_dev(gf_context *c, const gf_file *f, const uint8_t *dImage, size_t imageBytes, int elem, const gf_interp_spec *spec,
                                    size_t nPoints, const double *dRows, const double *dCols, const double *dColSpacing, int verifyChecksum,
                                    size_t maxTiles, const gf_interp_out *out, size_t *nTouched)
{
    if (!c || !f || !dImage || !nTouched || elem < 0 || (nPoints && (!dRows || !dCols))) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK || (s = interpOutArgs(spec, out)) != GF_OK) return s;
    PointsWhat w{};
    if ((s = pointsSpecArgs(i, spec, elem, dColSpacing != nullptr, w.ig)) != GF_OK) return s;
    int codecs[255];
    uint32_t fill[GF_MAX_ELEMS];
    if ((s = pointsFileArgs(c, i, dImage, imageBytes, true, nPoints, maxTiles, codecs, fill)) != GF_OK) return s;
    w.windows = true, w.nPoints = nPoints, w.elem = elem, w.rowsD = dRows, w.colsD = dCols, w.colSpacing = dColSpacing;
    w.out.z = out->z, w.out.zx = out->zx, w.out.zy = out->zy, w.out.zxx = out->zxx, w.out.zxy = out->zxy, w.out.zyy = out->zyy;
    w.out.normal = out->normal, w.out.status = out->status;
    return pointsDev(c, i, dImage, imageBytes, codecs, fill, verifyChecksum, maxTiles, w, nTouched);
}

gf_status gf_file_interp_coords_tiles(const gf_file *f, int kind, const gf_interp_spec *spec, size_t nPoints, const double *a, const double *b,
                                      int32_t *tiles, size_t tilesCap, size_t *nTiles)
{
    if (!f || !spec || !nTiles || (kind != GF_COORDS_GRID && kind != GF_COORDS_FILE) || (nPoints && (!a || !b)) || (tilesCap && !tiles)) return GF_ERR_ARG;
    *nTiles = 0;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    GfInterpGeom ig;
    if ((s = pointsSpecArgs(i, spec, -1, true, ig)) != GF_OK) return s;
    if (gfTilesOfGrid(i.grid).count() > POINTS_MAX_TILES_GRID) return GF_ERR_UNSUPPORTED;
    *nTiles = listBits(coordsBits(gridOf(i), ig, coordsOf(i), kind, nPoints, a, b), tiles, tilesCap);
    return GF_OK;
}

gf_status gf_file_interp_coords_dev(gf_context *c, const gf_file *f, const uint8_t *dImage, size_t imageBytes, int elem, int kind,
                                    const gf_interp_spec *spec, size_t nPoints, const double *dA, const double *dB, const double *dColSpacing,
                                    int verifyChecksum, size_t maxTiles, const gf_interp_out *out, double *dColSpacingUsed, size_t *nTouched)
{
    if (!f || !dImage || !nTouched || elem < 0 || (kind != GF_COORDS_GRID && kind != GF_COORDS_FILE) || (nPoints && (!dA || !dB))) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK || (s = interpOutArgs(spec, out)) != GF_OK) return s;
    PointsWhat w{};
    // (a geographic file's spacing comes from the rule unless the caller brings one: a zero du is refused either way, as a zero
    // col_spacing without per-point spacings is)
    if ((s = pointsSpecArgs(i, spec, elem, dColSpacing != nullptr, w.ig)) != GF_OK) return s;
    if (!c) return pointsNoContext(i, dImage, imageBytes, true);
    int codecs[255];
    uint32_t fill[GF_MAX_ELEMS];
    if ((s = pointsFileArgs(c, i, dImage, imageBytes, true, nPoints, maxTiles, codecs, fill)) != GF_OK) return s;
    w.windows = true, w.nPoints = nPoints, w.elem = elem, w.rowsD = dA, w.colsD = dB, w.colSpacing = dColSpacing;
    w.coords = true, w.kind = kind, w.co = coordsOf(i), w.spacingUsed = dColSpacingUsed;
    w.out.z = out->z, w.out.zx = out->zx, w.out.zy = out->zy, w.out.zxx = out->zxx, w.out.zxy = out->zxy, w.out.zyy = out->zyy;
    w.out.normal = out->normal, w.out.status = out->status;
    return pointsDev(c, i, dImage, imageBytes, codecs, fill, verifyChecksum, maxTiles, w, nTouched);
}

gf_status gf_file_interp_coords(gf_context *c, const gf_file *f, const uint8_t *image, size_t imageBytes, int elem, int kind,
                                const gf_interp_spec *spec, size_t nPoints, const double *a, const double *b, const double *colSpacing,
                                int verifyChecksum, size_t maxTiles, const gf_interp_out *out, double *colSpacingUsed, size_t *nTouched)
{
    if (!f || !image || !nTouched || elem < 0 || (kind != GF_COORDS_GRID && kind != GF_COORDS_FILE) || (nPoints && (!a || !b))) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK || (s = interpOutArgs(spec, out)) != GF_OK) return s;
    PointsWhat w{};
    if ((s = pointsSpecArgs(i, spec, elem, colSpacing != nullptr, w.ig)) != GF_OK) return s;
    if (!c) return pointsNoContext(i, image, imageBytes, false);
    int codecs[255];
    uint32_t fill[GF_MAX_ELEMS];
    if ((s = pointsFileArgs(c, i, image, imageBytes, false, nPoints, maxTiles, codecs, fill)) != GF_OK) return s;
    w.windows = true, w.nPoints = nPoints, w.elem = elem;
    w.coords = true, w.kind = kind, w.co = coordsOf(i);
    double *const host[6] = {out->z, out->zx, out->zy, out->zxx, out->zxy, out->zyy};
    int aP = 0, bP = 0, csP = 0, devP[6], normalP = 0, statusP = 0, usedP = 0;
    return pointsHost(
        c, i, image, imageBytes, codecs, fill, verifyChecksum, maxTiles, coordsBits(gridOf(i), w.ig, w.co, kind, nPoints, a, b), w, nTouched,
        [&](HostStage &sg) {
            aP = sg.in(a, nPoints * 8), bP = sg.in(b, nPoints * 8), csP = sg.in(colSpacing, nPoints * 8);
            for (int k = 0; k < 6; k++) devP[k] = sg.out(host[k], nPoints * 8);
            normalP = sg.out(out->normal, nPoints * 24), statusP = sg.out(out->status, nPoints * 4);
            usedP = sg.out(colSpacingUsed, nPoints * 8);
        },
        [&](HostStage &sg, PointsWhat &p) {
            p.rowsD = sg.ptr<double>(aP), p.colsD = sg.ptr<double>(bP), p.colSpacing = sg.ptr<double>(csP);
            p.out.z = sg.ptr<double>(devP[0]), p.out.zx = sg.ptr<double>(devP[1]), p.out.zy = sg.ptr<double>(devP[2]);
            p.out.zxx = sg.ptr<double>(devP[3]), p.out.zxy = sg.ptr<double>(devP[4]), p.out.zyy = sg.ptr<double>(devP[5]);
            p.out.normal = sg.ptr<double>(normalP), p.out.status = sg.ptr<int32_t>(statusP);
            p.spacingUsed = sg.ptr<double>(usedP);
        });
}

gf_status gf_file_read_points_elems(gf_context *c, const gf_file *f, const uint8_t *image, size_t imageBytes, size_t nPoints, const int32_t *rows,
                                    const int32_t *cols, int verifyChecksum, size_t maxTiles, void *const *values, int32_t *status,
                                    size_t *nTouched)
{
    if (!c || !f || !image || !values || !status || !nTouched || (nPoints && (!rows || !cols))) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK) return s;
    for (int e = 0; e < i.n_elems; e++)
        if (!values[e]) return GF_ERR_ARG;
    int codecs[255];
    uint32_t fill[GF_MAX_ELEMS];
    if ((s = pointsFileArgs(c, i, image, imageBytes, false, nPoints, maxTiles, codecs, fill)) != GF_OK) return s;
    PointsWhat w{};
    w.windows = false, w.nPoints = nPoints;
    int rowsP = 0, colsP = 0, valueP[GF_MAX_ELEMS], statusP = 0;
    void *dValues[GF_MAX_ELEMS];
    return pointsHost(
        c, i, image, imageBytes, codecs, fill, verifyChecksum, maxTiles, cellsBits(gridOf(i), nPoints, rows, cols), w, nTouched,
        [&](HostStage &sg) {
            rowsP = sg.in(rows, nPoints * 4), colsP = sg.in(cols, nPoints * 4);
            stageElems(sg, STAGE_OUT, i.elems, i.n_elems, nPoints, values, valueP);
            statusP = sg.out(status, (size_t)i.n_elems * nPoints * 4);
        },
        [&](HostStage &sg, PointsWhat &p) {
            sg.ptrs(valueP, i.n_elems, dValues);
            p.rowsI = sg.ptr<int32_t>(rowsP), p.colsI = sg.ptr<int32_t>(colsP), p.values = dValues, p.status = sg.ptr<int32_t>(statusP);
        });
}

gf_status gf_file_interp_points(gf_context *c, const gf_file *f, const uint8_t *image, size_t imageBytes, int elem, const gf_interp_spec *spec,
                                size_t nPoints, const double *rows, const double *cols, const double *colSpacing, int verifyChecksum,
                                size_t maxTiles, const gf_interp_out *out, size_t *nTouched)
{
    if (!c || !f || !image || !nTouched || elem < 0 || (nPoints && (!rows || !cols))) return GF_ERR_ARG;
    gf_file_info i;
    gf_status s = gf_file_get_info(f, &i);
    if (s != GF_OK || (s = interpOutArgs(spec, out)) != GF_OK) return s;
    PointsWhat w{};
    if ((s = pointsSpecArgs(i, spec, elem, colSpacing != nullptr, w.ig)) != GF_OK) return s;
    int codecs[255];
    uint32_t fill[GF_MAX_ELEMS];
    if ((s = pointsFileArgs(c, i, image, imageBytes, false, nPoints, maxTiles, codecs, fill)) != GF_OK) return s;
    w.windows = true, w.nPoints = nPoints, w.elem = elem;
    double *const host[6] = {out->z, out->zx, out->zy, out->zxx, out->zxy, out->zyy};
    int rowsP = 0, colsP = 0, csP = 0, devP[6], normalP = 0, statusP = 0;
    return pointsHost(
        c, i, image, imageBytes, codecs, fill, verifyChecksum, maxTiles, windowsBits(gridOf(i), w.ig, nPoints, rows, cols), w, nTouched,
        [&](HostStage &sg) {
            rowsP = sg.in(rows, nPoints * 8), colsP = sg.in(cols, nPoints * 8), csP = sg.in(colSpacing, nPoints * 8);
            for (int k = 0; k < 6; k++) devP[k] = sg.out(host[k], nPoints * 8);
            normalP = sg.out(out->normal, nPoints * 24), statusP = sg.out(out->status, nPoints * 4);
        },
        [&](HostStage &sg, PointsWhat &p) {
            p.rowsD = sg.ptr<double>(rowsP), p.colsD = sg.ptr<double>(colsP), p.colSpacing = sg.ptr<double>(csP);
            p.out.z = sg.ptr<double>(devP[0]), p.out.zx = sg.ptr<double>(devP[1]), p.out.zy = sg.ptr<double>(devP[2]);
            p.out.zxx = sg.ptr<double>(devP[3]), p.out.zxy = sg.ptr<double>(devP[4]), p.out.zyy = sg.ptr<double>(devP[5]);
            p.out.normal = sg.ptr<double>(normalP), p.out.status = sg.ptr<int32_t>(statusP);
        });
}

gf_status gf_file_update_points_elems_dev(gf_context *c, const gf_file_update *u, size_t nPoints, const int32_t *dRows, const int32_t *dCols,
                                          const void *const *dValues, size_t maxTiles, int flags, int64_t timeModified, uint8_t *dImage,
                                          size_t imageCap, uint64_t *dImageBytes, int32_t *dFileStatus, int32_t *dPointStatus,
                                          int32_t *dTileIndices, int32_t *dTileStatus, uint8_t *dCodecUsed, size_t *nTouched)
{
    if (!c || !u || !dValues || !dImage || ((uintptr_t)dImage & 7) != 0 || !dImageBytes || !dFileStatus || !dPointStatus || !dTileIndices ||
        !dTileStatus || !nTouched || (nPoints && (!dRows || !dCols))) return GF_ERR_ARG;
    *nTouched = 0;
    const GfFileUpdate &h = fileUpdateOf(u);
    const gf_file_info &i = h.info;
    int codecs[255];
    size_t maxRecord;
    gf_status s = pointsWriteArgs(c, h, dImage, imageCap, true, nPoints, maxTiles, dValues, codecs, maxRecord);
    if (s != GF_OK) return s;
    if (!deviceList(i.codecs, i.n_codecs, i.elems, i.n_elems)) return GF_ERR_UNSUPPORTED;
    if (nPoints == 0) return GF_OK;                                               // (nothing is enqueued: the image is not even closed anew)
    const GfPointsGrid g = gridOf(i);
    if (maxTiles > (size_t)g.nTilesGrid) maxTiles = (size_t)g.nTilesGrid;         // (no set of points touches more)
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    PointsBuf b;
    if ((s = pointsBuf(c, g, i.n_elems, maxTiles, true, b)) != GF_OK) return s;
    if ((s = c->hRecCounts.ensure(256 * 4)) != GF_OK) return s;
    PointsWhat w{};
    w.windows = false, w.nPoints = nPoints, w.rowsI = dRows, w.colsI = dCols;
    if ((s = pointsMarkRank(st, g, w, b, maxTiles)) != GF_OK) return s;
    // the first synchronisation: the host sizes pool, planes and the records' room by the count
    GF_HIP(hipMemcpyAsync(c->hRecCounts.p, b.count, 4, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    const size_t n = *(const uint32_t *)c->hRecCounts.p;
    *nTouched = n;
    if (n > maxTiles) return GF_ERR_CAPACITY;                                     // (no output and no byte of the image has been written)
    GfFileLocateArgs a{};
    a.image = dImage, a.imageBytes = h.imageBytes, a.dir = gfFileDirOf(i);
    a.starts = b.starts, a.ends = b.ends, a.verdict = b.verdict;
    a.tileList = b.list, a.nList = (uint32_t)n;
    GF_HIP(gf_launch_file_locate(a, st));
    GF_HIP(gf_launch_points_heads(GfPointsHeadsArgs{dImage, h.imageBytes, b.starts, b.ends, b.verdict, (uint32_t)n}, st));
    Carve kb;
    const size_t blobAt = kb.add(n * maxRecord), offsetsAt = kb.add((n + 1) * 8);
    if ((s = c->dFileUpdateBlob.ensure(kb)) != GF_OK) return s;
    uint8_t *dBlob = c->dFileUpdateBlob.at<uint8_t>(blobAt);
    uint64_t *dOffsets = c->dFileUpdateBlob.at<uint64_t>(offsetsAt);
    void *dPool[GF_MAX_ELEMS];
    const int32_t *dPre = nullptr;
    // (the second synchronisation is the records' pipeline's, inside)
    s = pointsWriteCells(c, st, i, g, n, dImage, (size_t)h.imageBytes, b.starts, b.ends, b.verdict, b, b.list, nPoints, dRows, dCols, dValues,
                         dPointStatus, dTileIndices, dPool, &dPre);
    if (s != GF_OK) return s;
    if (n) {
        s = recordsEncodeDev(c, st, i.codecs, i.n_codecs, i.elems, i.n_elems, g.nRowsTile, g.nColsTile, n, dTileIndices, (const void *const *)dPool,
                             i.checksum_enabled, dBlob, n * maxRecord, dOffsets, dCodecUsed, dTileStatus, dPre);
        if (s != GF_OK) return s;
    } else GF_HIP(hipMemsetAsync(dOffsets, 0, 8, st));                            // (every point lies outside the grid: the file is closed anew)
    // the allocator takes the records in ascending tile index; a tile with a negative status stays, record and entry
    return updateRecordsDev(c, h, dImage, imageCap, dBlob, dOffsets, dTileIndices, dTileStatus, dTileStatus, n, n * maxRecord, timeModified, flags, 0,
                            dImageBytes, dFileStatus);
}

gf_status gf_file_update_points_elems(gf_context *c, const gf_file_update *u, size_t nPoints, const int32_t *rows, const int32_t *cols,
                                      const void *const *values, size_t maxTiles, int flags, int64_t timeModified, uint8_t *image, size_t imageCap,
                                      uint64_t *imageBytes, int32_t *pointStatus, int32_t *tileIndices, int32_t *tileStatus, uint8_t *codecUsed,
                                      size_t *nTouched)
{
    if (!c || !u || !values || !image || !imageBytes || !pointStatus || !tileIndices || !tileStatus || !nTouched || (nPoints && (!rows || !cols)))
        return GF_ERR_ARG;
    *nTouched = 0;
    const GfFileUpdate &h = fileUpdateOf(u);
    const gf_file_info &i = h.info;
    *imageBytes = h.imageBytes;
    int codecs[255];
    size_t maxRecord;
    gf_status s = pointsWriteArgs(c, h, image, imageCap, false, nPoints, maxTiles, values, codecs, maxRecord);
    if (s != GF_OK) return s;
    if (nPoints == 0) return GF_OK;                                               // (the image is not even closed anew)
    const GfPointsGrid g = gridOf(i);
    const std::vector<uint32_t> bits = cellsBits(g, nPoints, rows, cols);
    const size_t n = listBits(bits, nullptr, 0);
    *nTouched = n;
    if (n > maxTiles) return GF_ERR_CAPACITY;
    if (n == 0) {                                                                 // every point lies outside the grid: the file is closed anew
        for (size_t k = 0; k < (size_t)i.n_elems * nPoints; k++) pointStatus[k] = GF_ERR_ARG;
        const uint64_t none = 0;
        return gfFileUpdateAssemble(h, image, imageCap, nullptr, &none, nullptr, nullptr, 0, timeModified, flags, imageBytes);
    }
    // the touched tiles' old records, looked up and judged by their heads as gf_file_update_block_elems judges them, staged end to end
    std::vector<int32_t> list(n), verdict(n);
    listBits(bits, list.data(), n);
    std::vector<uint64_t> from, starts(n, 0), ends(n, 0);
    uint64_t oldBytes = 0;
    const GfFileDir dir = gfFileDirOf(i);
    for (size_t k = 0; k < n; k++) {
        uint64_t pos, size = 0;
        uint32_t sizeWord;
        int32_t v = gfFileLocate(dir, image, h.imageBytes, list[k], &pos, &sizeWord);
        if (v == GF_OK && pos != 0) {
            v = gfFsRecordHead(h.imageBytes, i.content_pos, pos, GF_FILE_REC_TILE, 24, &size, GfLoadLe{image});
            if (v == GF_OK) {
                v = GF_FILE_LOCATED;
                from.push_back(pos - 8);
                starts[k] = oldBytes, ends[k] = oldBytes + size;
                oldBytes += size;
            }
        }
        verdict[k] = v;
    }
    std::vector<uint8_t> old((size_t)oldBytes + 16);
    for (size_t k = 0, r = 0; k < n; k++)
        if (verdict[k] == GF_FILE_LOCATED) memcpy(old.data() + starts[k], image + from[r++], (size_t)(ends[k] - starts[k]));
    const bool onDevice = deviceList(i.codecs, i.n_codecs, i.elems, i.n_elems);
    const size_t maxBlob = n * maxRecord;
    std::vector<uint8_t> blob(maxBlob + 16);
    std::vector<uint64_t> offsets(n + 1, 0);
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    PointsBuf b;
    if ((s = pointsBuf(c, g, i.n_elems, n, false, b)) != GF_OK) return s;
    // staging: the old records | starts | ends | verdicts | the list | rows | cols | the values of element 0, 1, ... | the points'
    // statuses | tile indices, and for a device list the records at their largest | offsets | the tiles' statuses | codec used
    HostStage sg(c);
    const int oldP = sg.in(old.data(), (size_t)oldBytes, 32), startsP = sg.in(starts.data(), n * 8), endsP = sg.in(ends.data(), n * 8);
    const int verdictP = sg.in(verdict.data(), n * 4), listP = sg.in(list.data(), n * 4);
    const int rowsP = sg.in(rows, nPoints * 4), colsP = sg.in(cols, nPoints * 4);
    int valueP[GF_MAX_ELEMS];
    stageElems(sg, STAGE_IN, i.elems, i.n_elems, nPoints, values, valueP);
    const int pointP = sg.out(pointStatus, (size_t)i.n_elems * nPoints * 4);
    HostWriteParts parts;
    parts.indices = sg.out(tileIndices, n * 4);
    parts.blob = sg.held(blob.data(), onDevice ? maxBlob : 0), parts.offsets = sg.out(onDevice ? offsets.data() : nullptr, (n + 1) * 8);
    parts.status = sg.out(onDevice ? tileStatus : nullptr, n * 4), parts.used = sg.out(onDevice ? codecUsed : nullptr, (size_t)i.n_elems * n);
    if ((s = sg.begin()) != GF_OK) return s;
    // the slots of the tiles on the device come from the device's own bitmap of the staged points
    PointsWhat w{};
    w.windows = false, w.nPoints = nPoints, w.rowsI = sg.ptr<int32_t>(rowsP), w.colsI = sg.ptr<int32_t>(colsP);
    if ((s = pointsMarkRank(st, g, w, b, 0)) != GF_OK) return s;
    void *dValues[GF_MAX_ELEMS], *dPool[GF_MAX_ELEMS];
    sg.ptrs(valueP, i.n_elems, dValues);
    const int32_t *dPre = nullptr;
    s = pointsWriteCells(c, st, i, g, n, sg.ptr<uint8_t>(oldP), (size_t)oldBytes, sg.ptr<uint64_t>(startsP), sg.ptr<uint64_t>(endsP),
                         sg.ptr<int32_t>(verdictP), b, sg.ptr<int32_t>(listP), nPoints, w.rowsI, w.colsI, dValues, sg.ptr<int32_t>(pointP),
                         sg.ptr<int32_t>(parts.indices), dPool, &dPre);
    if (s != GF_OK) return s;
    s = hostWriteTail(c, sg, parts, onDevice, i.codecs, i.n_codecs, i.elems, i.n_elems, g.nRowsTile, g.nColsTile, n, (const void *const *)dPool, dPre,
                      i.checksum_enabled, maxBlob, blob.data(), maxBlob, offsets.data(), tileIndices, codecUsed, tileStatus);
    if (s == GF_ERR_ARG || s == GF_ERR_UNSUPPORTED || s == GF_ERR_HIP || s == GF_ERR_CAPACITY) return s;   // (not a tile's verdict)
    gf_status first = GF_OK;
    for (size_t k = 0; k < n && first == GF_OK; k++)
        if (tileStatus[k] < 0) first = (gf_status)tileStatus[k];
    s = gfFileUpdateAssemble(h, image, imageCap, blob.data(), offsets.data(), tileIndices, tileStatus, n, timeModified, flags, imageBytes);
    return s != GF_OK ? s : first;                                // (a refusal of the whole update comes before a tile's status)
}

}  // extern "C"
