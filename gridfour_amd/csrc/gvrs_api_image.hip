// gvrs_api_image.hip -- ARGB images as element planes and as overviews: packed words split into the planes r, g, b or Y, Co, Cg and
// joined from them (gf_image_split[_dev], gf_image_join[_dev]), an image reduced by an integer factor (gf_image_reduce[_dev],
// gf_image_reduce_size), and the two composed with the block write and the block read: pixels to tile records of three elements
// and back (gf_image_write[_dev], gf_image_read[_dev]).  The plain device forms check their arguments, fill in the kernels'
// arguments and launch (gvrs_image.hip; the reduce: gvrs_downsample.hip): they allocate nothing and never synchronise.  None of
// the calls takes a stream: they run on the context's, and the launch helpers below take the stream as an argument.
// Reference: demo/src/main/java/org/gridfour/demo/imaging/ExperimentalImageStorage.java:203-213, :242-256, :275-286;
// demo/src/main/java/org/gridfour/demo/geoTiff/DemoCOG.java:735-770.

#include "gvrs_api_internal.h"

#include <climits>

namespace {

constexpr size_t IMG_MAX_PIXELS = (size_t)1 << 48;

bool modelOk(int model) { return model == GF_IMAGE_RGB || model == GF_IMAGE_YCOCG; }
bool typeOk(int elemType) { return elemType == GF_ELEM_INT || elemType == GF_ELEM_SHORT; }
bool fillOk(int elemType, int32_t fillI) { return elemType != GF_ELEM_SHORT || (fillI >= -32768 && fillI <= 32767); }
size_t itemBytes(int elemType) { return elemType == GF_ELEM_SHORT ? 2 : 4; }

// what the host can check of a split or a join; onDevice: the pointers' alignment counts
gf_status planeArgs(const gf_context *c, int model, int elemType, size_t nPixels, const void *argb, const void *const *planes, bool onDevice)
{
    if (!c || !argb || !planes || !planes[0] || !planes[1] || !planes[2]) return GF_ERR_ARG;
    if (!modelOk(model) || !typeOk(elemType)) return GF_ERR_ARG;
    if (onDevice) {
        if ((uintptr_t)argb & 3u) return GF_ERR_ARG;
        for (int k = 0; k < 3; k++)
            if ((uintptr_t)planes[k] & (itemBytes(elemType) - 1)) return GF_ERR_ARG;
    }
    return nPixels > IMG_MAX_PIXELS ? GF_ERR_UNSUPPORTED : GF_OK;
}

// width, height and factor alone: ARG, UNSUPPORTED or the reduced size
gf_status reduceSize(int width, int height, int factor, int &outWidth, int &outHeight)
{
    if (width < 1 || height < 1 || factor < 1) return GF_ERR_ARG;
    if (factor > GF_IMAGE_MAX_FACTOR) return GF_ERR_UNSUPPORTED;
    if ((uint64_t)width * (uint64_t)height > IMG_MAX_PIXELS) return GF_ERR_UNSUPPORTED;
    outWidth = width / factor, outHeight = height / factor;
    return GF_OK;
}

gf_status reduceArgs(const gf_context *c, int width, int height, int factor, const void *argb, const void *out, bool onDevice, int &outWidth,
                     int &outHeight)
{
    if (!c || !argb || !out) return GF_ERR_ARG;
    if (onDevice && (((uintptr_t)argb | (uintptr_t)out) & 3u)) return GF_ERR_ARG;
    return reduceSize(width, height, factor, outWidth, outHeight);
}

// the launch helpers (the caller holds the lock, has checked the arguments and has set the device)
gf_status splitLaunch(hipStream_t st, int model, int elemType, size_t nPixels, const int32_t *dArgb, void *const *dPlanes)
{
    GfImageArgs a{};
    a.model = model, a.elemType = elemType, a.nPixels = nPixels, a.argb = dArgb;
    for (int k = 0; k < 3; k++) a.planes[k] = dPlanes[k];
    GF_HIP(gf_launch_image_split(a, st));
    return GF_OK;
}

gf_status joinLaunch(hipStream_t st, int model, int elemType, size_t nPixels, const void *const *dPlanes, int32_t *dArgb)
{
    GfImageArgs a{};
    a.model = model, a.elemType = elemType, a.nPixels = nPixels, a.argb = dArgb;
    for (int k = 0; k < 3; k++) a.planes[k] = dPlanes[k];
    GF_HIP(gf_launch_image_join(a, st));
    return GF_OK;
}

gf_status reduceLaunch(hipStream_t st, int width, int factor, int outWidth, int outHeight, const int32_t *dArgb, int32_t *dOut)
{
    GfDownsampleArgs a{};
    a.g.pitch = width;
    a.g.outRows = outHeight, a.g.outCols = outWidth;
    a.g.f = factor;
    a.g.elemType = GF_DS_ARGB;
    a.block = dArgb, a.out = dOut;
    GF_HIP(gf_launch_downsample(a, GF_DS_AUTO, st));
    return GF_OK;
}

// the three elements of an image's records, and the whole range of their type
void imageElems(int elemType, int32_t fillI, gf_elem_spec *elems, gf_elem_range *ranges)
{
    for (int k = 0; k < 3; k++) {
        elems[k] = gf_elem_spec{};
        elems[k].type = elemType, elems[k].fill_i = fillI;
        ranges[k] = gf_elem_range{};
        ranges[k].min_i = elemType == GF_ELEM_SHORT ? -32768 : INT_MIN, ranges[k].max_i = elemType == GF_ELEM_SHORT ? 32767 : INT_MAX;
    }
}

// what a record form adds to the block call's own checks
gf_status recordFormArgs(int model, int elemType, int32_t fillI, const void *argb, bool onDevice)
{
    if (!argb || !modelOk(model) || !typeOk(elemType) || !fillOk(elemType, fillI)) return GF_ERR_ARG;
    if (onDevice && ((uintptr_t)argb & 3u)) return GF_ERR_ARG;
    return GF_OK;
}

// three planes of nPixels items in a buffer of the context
gf_status planeArrays(DevBuf &b, int elemType, size_t nPixels, void **planes)
{
    Carve k;
    size_t at[3];
    for (int e = 0; e < 3; e++) at[e] = k.add(nPixels * itemBytes(elemType) + 4);
    const gf_status s = b.ensure(k);
    for (int e = 0; e < 3 && s == GF_OK; e++) planes[e] = b.at<void>(at[e]);
    return s;
}

}  // namespace

extern "C" {

gf_status gf_image_split_dev(gf_context *c, int model, int elemType, size_t nPixels, const int32_t *dArgb, void *const *dPlanes)
{
    const gf_status s = planeArgs(c, model, elemType, nPixels, dArgb, dPlanes, true);
    if (s != GF_OK || nPixels == 0) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return splitLaunch(c->stream, model, elemType, nPixels, dArgb, dPlanes);
}

gf_status gf_image_join_dev(gf_context *c, int model, int elemType, size_t nPixels, const void *const *dPlanes, int32_t *dArgb)
{
    const gf_status s = planeArgs(c, model, elemType, nPixels, dArgb, dPlanes, true);
    if (s != GF_OK || nPixels == 0) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return joinLaunch(c->stream, model, elemType, nPixels, dPlanes, dArgb);
}

gf_status gf_image_reduce_size(int width, int height, int factor, int *outWidth, int *outHeight)
{
    if (!outWidth || !outHeight) return GF_ERR_ARG;
    int w = 0, h = 0;
    const gf_status s = reduceSize(width, height, factor, w, h);
    if (s == GF_OK) *outWidth = w, *outHeight = h;
    return s;
}

gf_status gf_image_reduce_dev(gf_context *c, int width, int height, int factor, const int32_t *dArgb, int32_t *dOut)
{
    int ow = 0, oh = 0;
    const gf_status s = reduceArgs(c, width, height, factor, dArgb, dOut, true, ow, oh);
    if (s != GF_OK || ow == 0 || oh == 0) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return reduceLaunch(c->stream, width, factor, ow, oh, dArgb, dOut);
}

gf_status gf_image_split(gf_context *c, int model, int elemType, size_t nPixels, const int32_t *argb, void *const *planes)
{
    gf_status s = planeArgs(c, model, elemType, nPixels, argb, planes, false);
    if (s != GF_OK || nPixels == 0) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: the words | the three planes (four spare bytes behind each, as the record forms' planes have)
    HostStage sg(c);
    int planeP[3];
    const int argbP = sg.in(argb, nPixels * 4);
    for (int k = 0; k < 3; k++) planeP[k] = sg.add(planes[k], nPixels * itemBytes(elemType), STAGE_OUT, 4);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dPlanes[3];
    sg.ptrs(planeP, 3, dPlanes);
    return (s = splitLaunch(c->stream, model, elemType, nPixels, sg.ptr<int32_t>(argbP), dPlanes)) != GF_OK ? s : sg.end();
}

gf_status gf_image_join(gf_context *c, int model, int elemType, size_t nPixels, const void *const *planes, int32_t *argb)
{
    gf_status s = planeArgs(c, model, elemType, nPixels, argb, planes, false);
    if (s != GF_OK || nPixels == 0) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: the three planes (four spare bytes behind each) | the words
    HostStage sg(c);
    int planeP[3];
    for (int k = 0; k < 3; k++) planeP[k] = sg.in(planes[k], nPixels * itemBytes(elemType), 4);
    const int argbP = sg.out(argb, nPixels * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dPlanes[3];
    sg.ptrs(planeP, 3, dPlanes);
    return (s = joinLaunch(c->stream, model, elemType, nPixels, dPlanes, sg.ptr<int32_t>(argbP))) != GF_OK ? s : sg.end();
}

gf_status gf_image_reduce(gf_context *c, int width, int height, int factor, const int32_t *argb, int32_t *out)
{
    int ow = 0, oh = 0;
    gf_status s = reduceArgs(c, width, height, factor, argb, out, false, ow, oh);
    if (s != GF_OK || ow == 0 || oh == 0) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: the image | the reduced image
    HostStage sg(c);
    const int inP = sg.in(argb, (size_t)width * (size_t)height * 4), outP = sg.out(out, (size_t)ow * (size_t)oh * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    return (s = reduceLaunch(c->stream, width, factor, ow, oh, sg.ptr<int32_t>(inP), sg.ptr<int32_t>(outP))) != GF_OK ? s : sg.end();
}

gf_status gf_image_write_dev(gf_context *c, const int *codecs, int nCodecs, int model, int elemType, int32_t fillI, const gf_grid_spec *grid,
                             const gf_rect *rect, const int32_t *dArgb, size_t nOld, const uint8_t *dOldBlob, size_t oldBlobBytes,
                             const uint64_t *dOldOffsets, int verifyOldChecksum, int checksumEnabled, uint8_t *dBlob, size_t blobCap,
                             uint64_t *dOffsets, int32_t *dTileIndices, uint8_t *dCodecUsed, int32_t *dStatus)
{
    gf_status s = recordFormArgs(model, elemType, fillI, dArgb, true);
    if (s != GF_OK) return s;
    gf_elem_spec elems[3];
    gf_elem_range ranges[3];
    imageElems(elemType, fillI, elems, ranges);
    const void *standIn[3] = {dArgb, dArgb, dArgb};                             // (the planes are the context's: checked as non-null and aligned)
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    s = blockWriteArgs(c, codecs, nCodecs, elems, ranges, 3, grid, rect, standIn, nOld, dOldBlob, dOldOffsets, dBlob, blobCap, dOffsets, dTileIndices,
                       dStatus, true, g, cut);
    if (s != GF_OK) return s;
    if (!deviceList(codecs, nCodecs, elems, 3)) return GF_ERR_UNSUPPORTED;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const size_t nPixels = (size_t)rect->n_rows * (size_t)rect->n_cols;
    void *dPlanes[3];
    if ((s = planeArrays(c->dImage, elemType, nPixels, dPlanes)) != GF_OK) return s;
    if ((s = splitLaunch(c->stream, model, elemType, nPixels, dArgb, dPlanes)) != GF_OK) return s;
    return blockWriteDev(c, c->stream, codecs, nCodecs, elems, 3, g, cut, dPlanes, nOld, dOldBlob, oldBlobBytes, dOldOffsets, verifyOldChecksum,
                         checksumEnabled, dBlob, blobCap, dOffsets, dTileIndices, dCodecUsed, dStatus);
}

gf_status gf_image_read_dev(gf_context *c, const int *codecs, int nCodecs, int model, int elemType, int32_t fillI, const gf_grid_spec *grid,
                            const gf_rect *rect, size_t nRecords, const uint8_t *dBlob, size_t blobBytes, const uint64_t *dOffsets,
                            int verifyChecksum, int32_t *dArgb, int32_t *dStatus)
{
    gf_status s = recordFormArgs(model, elemType, fillI, dArgb, true);
    if (s != GF_OK) return s;
    gf_elem_spec elems[3];
    gf_elem_range ranges[3];
    imageElems(elemType, fillI, elems, ranges);
    void *standIn[3] = {dArgb, dArgb, dArgb};
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    s = blockReadArgs(c, codecs, nCodecs, elems, 3, grid, rect, nRecords, dBlob, true, dOffsets, standIn, dStatus, g, fill);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const size_t nPixels = (size_t)rect->n_rows * (size_t)rect->n_cols;
    void *dPlanes[3];
    if ((s = planeArrays(c->dImage, elemType, nPixels, dPlanes)) != GF_OK) return s;
    s = blockReadDev(c, c->stream, codecs, nCodecs, elems, 3, g, fill, nRecords, dBlob, blobBytes, dOffsets, verifyChecksum, dPlanes, dStatus);
    if (s != GF_OK) return s;
    return joinLaunch(c->stream, model, elemType, nPixels, dPlanes, dArgb);
}

// The host forms of the record calls: the split and the join run on the device through the host forms above, the records go through
// gf_block_write_elems / gf_block_read_elems, which stage them and take any codec list.  Each of the two calls takes the lock for
// itself: between them the planes lie in host memory of this call.
gf_status gf_image_write(gf_context *c, const int *codecs, int nCodecs, int model, int elemType, int32_t fillI, const gf_grid_spec *grid,
                         const gf_rect *rect, const int32_t *argb, size_t nOld, const uint8_t *oldBlob, const uint64_t *oldOffsets,
                         int verifyOldChecksum, int checksumEnabled, uint8_t *blob, size_t blobCap, uint64_t *offsets, int32_t *tileIndices,
                         uint8_t *codecUsed, int32_t *status)
{
    gf_status s = recordFormArgs(model, elemType, fillI, argb, false);
    if (s != GF_OK) return s;
    gf_elem_spec elems[3];
    gf_elem_range ranges[3];
    imageElems(elemType, fillI, elems, ranges);
    const void *standIn[3] = {argb, argb, argb};
    GfBlockGeom g{};
    GfBlockCutElem cut[GF_MAX_ELEMS];
    s = blockWriteArgs(c, codecs, nCodecs, elems, ranges, 3, grid, rect, standIn, nOld, oldBlob, oldOffsets, blob, blobCap, offsets, tileIndices, status,
                       false, g, cut);
    if (s != GF_OK) return s;
    const size_t nPixels = (size_t)rect->n_rows * (size_t)rect->n_cols;
    std::vector<uint8_t> host[3];
    void *planes[3];
    for (int k = 0; k < 3; k++) {
        host[k].resize(nPixels * itemBytes(elemType) + 4);
        planes[k] = host[k].data();
    }
    if ((s = gf_image_split(c, model, elemType, nPixels, argb, planes)) != GF_OK) return s;
    return gf_block_write_elems(c, codecs, nCodecs, elems, ranges, 3, grid, rect, planes, nOld, oldBlob, oldOffsets, verifyOldChecksum, checksumEnabled,
                                blob, blobCap, offsets, tileIndices, codecUsed, status);
}

gf_status gf_image_read(gf_context *c, const int *codecs, int nCodecs, int model, int elemType, int32_t fillI, const gf_grid_spec *grid,
                        const gf_rect *rect, size_t nRecords, const uint8_t *blob, const uint64_t *offsets, int verifyChecksum, int32_t *argb,
                        int32_t *status)
{
    gf_status s = recordFormArgs(model, elemType, fillI, argb, false);
    if (s != GF_OK) return s;
    gf_elem_spec elems[3];
    gf_elem_range ranges[3];
    imageElems(elemType, fillI, elems, ranges);
    void *standIn[3] = {argb, argb, argb};
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    s = blockReadArgs(c, codecs, nCodecs, elems, 3, grid, rect, nRecords, blob, false, offsets, standIn, status, g, fill);
    if (s != GF_OK) return s;
    const size_t nPixels = (size_t)rect->n_rows * (size_t)rect->n_cols;
    std::vector<uint8_t> host[3];
    void *planes[3];
    for (int k = 0; k < 3; k++) {
        host[k].resize(nPixels * itemBytes(elemType) + 4);
        planes[k] = host[k].data();
    }
    if ((s = gf_block_read_elems(c, codecs, nCodecs, elems, 3, grid, rect, nRecords, blob, offsets, verifyChecksum, planes, status)) != GF_OK) return s;
    return gf_image_join(c, model, elemType, nPixels, planes, argb);
}

}  // extern "C"
