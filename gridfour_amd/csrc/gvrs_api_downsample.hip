// gvrs_api_downsample.hip -- a grid block averaged down by an integer factor: the loop of the reference's ExampleDownsample over
// blocks that lie in device memory (gf_block_downsample_elems_dev), in host memory (gf_block_downsample_elems, staged through the
// context) or still in tile records (gf_block_read_downsampled_elems[_dev]: the block read into a temporary of the context, then
// the same kernels), and the rectangle rule that goes with them (gf_block_downsample_rect).  The plain device form checks its
// arguments, fills in the kernels' arguments and launches (gf_launch_downsample, gvrs_downsample.hip), one launch per element:
// it allocates nothing and never synchronises.
// Reference: demo/src/main/java/org/gridfour/demo/globalDEM/ExampleDownsample.java:164-210, :228-239.

#include "gvrs_api_internal.h"

#ifdef GF_DIAG
// The diagnostic flavour of the library only, for tools/downsample_rate.py (loaded by name; not part of include/gvrs_hip_codec.h):
// GF_DS_DIRECT / GF_DS_STAGED for every later call of the process, GF_DS_AUTO to give the choice back.
static int g_dsPath = GF_DS_AUTO;
extern "C" __attribute__((visibility("default"))) void gf_internal_downsample_path(int path) { g_dsPath = path; }
#else
constexpr int g_dsPath = GF_DS_AUTO;
#endif

namespace {

constexpr int DS_MAX_FACTOR = 46340;            // f * f stays a Java int

// block and factor alone: ARG, UNSUPPORTED or the output rectangle
gf_status dsRect(const gf_rect *block, int factor, gf_rect &out)
{
    if (!block || factor < 1 || block->n_rows < 1 || block->n_cols < 1 || block->row0 < 0 || block->col0 < 0) return GF_ERR_ARG;
    if (factor > DS_MAX_FACTOR) return GF_ERR_UNSUPPORTED;
    gf_ds_axis(block->row0, block->n_rows, factor, out.row0, out.n_rows);
    gf_ds_axis(block->col0, block->n_cols, factor, out.col0, out.n_cols);
    return GF_OK;
}

// what the host can check of a plain call; fills the output rectangle.  icfAsCodes: an ICF element is taken as its INT codes
// (the record forms), else refused
gf_status dsArgs(const gf_context *c, const gf_elem_spec *elems, int nElems, const gf_rect *block, int factor, const void *const *blocks,
                 void *const *out, bool icfAsCodes, gf_rect &outRect)
{
    if (!c || !elems || !blocks || !out || nElems < 1 || nElems > GF_MAX_ELEMS) return GF_ERR_ARG;
    gf_status s = dsRect(block, factor, outRect);
    if (s == GF_ERR_ARG) return s;
    for (int e = 0; e < nElems; e++) {
        const int type = elems[e].type;
        if (type < GF_ELEM_INT || type > GF_ELEM_ICF) return GF_ERR_ARG;
        if (type == GF_ELEM_SHORT && (elems[e].fill_i < -32768 || elems[e].fill_i > 32767)) return GF_ERR_ARG;
        if (!blocks[e] || !out[e] || ((uintptr_t)blocks[e] & 3) != 0 || ((uintptr_t)out[e] & 3) != 0) return GF_ERR_ARG;
        if (type == GF_ELEM_ICF && !icfAsCodes) s = firstOf(s, GF_ERR_UNSUPPORTED);
    }
    return s;
}

// one launch per element (the caller holds the lock and has checked the arguments; the output rectangle is not empty)
gf_status dsLaunch(gf_context *c, hipStream_t st, const gf_elem_spec *elems, int nElems, const gf_rect &block, int factor, const gf_rect &outRect,
                   const void *const *dBlocks, void *const *dOut)
{
    GfDownsampleArgs a{};
    a.g.pitch = block.n_cols;
    a.g.outRows = outRect.n_rows, a.g.outCols = outRect.n_cols;
    a.g.rowOff = (int32_t)((int64_t)outRect.row0 * factor - block.row0), a.g.colOff = (int32_t)((int64_t)outRect.col0 * factor - block.col0);
    a.g.f = factor;
    for (int e = 0; e < nElems; e++) {
        a.g.elemType = elems[e].type == GF_ELEM_ICF ? GF_ELEM_INT : elems[e].type;
        a.g.fillI = elems[e].fill_i;
        a.block = dBlocks[e], a.out = dOut[e];
        GF_HIP(gf_launch_downsample(a, g_dsPath, st));
    }
    return GF_OK;
}

// the record forms' argument checks: the block read's on the elements as given, then the factor; asCodes: the elements with ICF
// turned into INT on fill_i, fill: their fills' bits
gf_status dsReadArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const gf_grid_spec *grid,
                     const gf_rect *rect, int factor, size_t nRecords, const uint8_t *blob, bool blobOnDevice, const uint64_t *offsets,
                     void *const *out, const int32_t *status, GfBlockGeom &g, gf_elem_spec *asCodes, uint32_t *fill, gf_rect &outRect)
{
    gf_status s = blockReadArgs(c, codecs, nCodecs, elems, nElems, grid, rect, nRecords, blob, blobOnDevice, offsets, out, status, g, fill);
    if (s == GF_ERR_ARG) return s;
    if (factor < 1) return GF_ERR_ARG;
    for (int e = 0; e < nElems; e++)
        if (((uintptr_t)out[e] & 3) != 0) return GF_ERR_ARG;
    s = firstOf(s, dsRect(rect, factor, outRect));
    if (s != GF_OK) return s;
    for (int e = 0; e < nElems; e++) {
        asCodes[e] = elems[e];
        if (elems[e].type == GF_ELEM_ICF) asCodes[e].type = GF_ELEM_INT;
    }
    return elemFills(asCodes, nElems, fill);
}

}  // namespace

extern "C" {

gf_status gf_block_downsample_rect(const gf_rect *block, int factor, gf_rect *out)
{
    if (!out) return GF_ERR_ARG;
    gf_rect r{};
    const gf_status s = dsRect(block, factor, r);
    if (s == GF_OK) *out = r;
    return s;
}

gf_status gf_block_downsample_elems_dev(gf_context *c, void *stream, const gf_elem_spec *elems, int nElems, const gf_rect *block, int factor,
                                        const void *const *dBlocks, void *const *dOut)
{
    gf_rect outRect{};
    const gf_status s = dsArgs(c, elems, nElems, block, factor, dBlocks, dOut, false, outRect);
    if (s != GF_OK) return s;
    if (outRect.n_rows == 0 || outRect.n_cols == 0) return GF_OK;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return dsLaunch(c, streamOf(c, stream), elems, nElems, *block, factor, outRect, dBlocks, dOut);
}

gf_status gf_block_downsample_elems(gf_context *c, const gf_elem_spec *elems, int nElems, const gf_rect *block, int factor,
                                    const void *const *blocks, void *const *out)
{
    gf_rect outRect{};
    gf_status s = dsArgs(c, elems, nElems, block, factor, blocks, out, false, outRect);
    if (s != GF_OK) return s;
    if (outRect.n_rows == 0 || outRect.n_cols == 0) return GF_OK;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: the elements' blocks, then their coarse blocks
    HostStage sg(c);
    int inP[GF_MAX_ELEMS], outP[GF_MAX_ELEMS];
    stageElems(sg, STAGE_IN, elems, nElems, (size_t)block->n_rows * (size_t)block->n_cols, blocks, inP);
    stageElems(sg, STAGE_OUT, elems, nElems, (size_t)outRect.n_rows * (size_t)outRect.n_cols, out, outP);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dBlocks[GF_MAX_ELEMS], *dOut[GF_MAX_ELEMS];
    sg.ptrs(inP, nElems, dBlocks), sg.ptrs(outP, nElems, dOut);
    return (s = dsLaunch(c, c->stream, elems, nElems, *block, factor, outRect, dBlocks, dOut)) != GF_OK ? s : sg.end();
}

gf_status gf_block_read_downsampled_elems_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems,
                                              const gf_grid_spec *grid, const gf_rect *rect, int factor, size_t nRecords, const uint8_t *dBlob,
                                              size_t blobBytes, const uint64_t *dOffsets, int verifyChecksum, void *const *dOut, int32_t *dStatus)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    gf_elem_spec asCodes[GF_MAX_ELEMS];
    gf_rect outRect{};
    gf_status s = dsReadArgs(c, codecs, nCodecs, elems, nElems, grid, rect, factor, nRecords, dBlob, true, dOffsets, dOut, dStatus, g, asCodes, fill,
                             outRect);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    void *dFull[GF_MAX_ELEMS];
    if ((s = elemArrays(c->dDsBlocks, asCodes, nElems, (size_t)rect->n_rows * (size_t)rect->n_cols, dFull)) != GF_OK) return s;   // at full resolution
    s = blockReadDev(c, stream, codecs, nCodecs, asCodes, nElems, g, fill, nRecords, dBlob, blobBytes, dOffsets, verifyChecksum, dFull, dStatus);
    if (s != GF_OK || outRect.n_rows == 0 || outRect.n_cols == 0) return s;
    return dsLaunch(c, streamOf(c, stream), asCodes, nElems, *rect, factor, outRect, dFull, dOut);
}

gf_status gf_block_read_downsampled_elems(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems,
                                          const gf_grid_spec *grid, const gf_rect *rect, int factor, size_t nRecords, const uint8_t *blob,
                                          const uint64_t *offsets, int verifyChecksum, void *const *out, int32_t *status)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    gf_elem_spec asCodes[GF_MAX_ELEMS];
    gf_rect outRect{};
    gf_status s = dsReadArgs(c, codecs, nCodecs, elems, nElems, grid, rect, factor, nRecords, blob, false, offsets, out, status, g, asCodes, fill,
                             outRect);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const size_t blobBytes = nRecords ? (size_t)offsets[nRecords] : 0;
    const size_t outCells = (size_t)outRect.n_rows * (size_t)outRect.n_cols;
    // staging: blob | offsets | the coarse block of element 0, 1, ... | statuses
    HostStage sg(c);
    int outP[GF_MAX_ELEMS];
    const int blobP = sg.in(blob, blobBytes, 32), offsetsP = sg.in(offsets, nRecords ? (nRecords + 1) * 8 : 0);
    stageElems(sg, STAGE_OUT, asCodes, nElems, outCells, out, outP);
    const int statusP = sg.out(status, (size_t)nElems * nRecords * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dFull[GF_MAX_ELEMS], *dOut[GF_MAX_ELEMS];
    sg.ptrs(outP, nElems, dOut);
    if ((s = elemArrays(c->dDsBlocks, asCodes, nElems, (size_t)rect->n_rows * (size_t)rect->n_cols, dFull)) != GF_OK) return s;   // at full resolution
    s = blockReadDev(c, c->stream, codecs, nCodecs, asCodes, nElems, g, fill, nRecords, sg.ptr<uint8_t>(blobP), blobBytes,
                     sg.ptr<uint64_t>(offsetsP), verifyChecksum, dFull, sg.ptr<int32_t>(statusP));
    if (s != GF_OK) return s;
    if (outCells && (s = dsLaunch(c, c->stream, asCodes, nElems, *rect, factor, outRect, dFull, dOut)) != GF_OK) return s;
    return sg.end();
}

}  // extern "C"
