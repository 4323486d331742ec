// gvrs_api_file.hip -- GVRS files: gf_file_open and its getters (the parser of gvrs_file_parse.h behind a handle; no device, no
// context) and the block reads from a file image: gf_file_read_block_elems_dev finds the records of the rectangle's tiles in the
// image where it lies in device memory (k_file_locate, gvrs_file.hip) and hands their extents to the records' pipeline of
// gvrs_api_blocks.hip; gf_file_read_block_elems looks them up on the host and stages only their records.
// Reference: gvrs/GvrsFile.java:341-483, gvrs/RecordManager.java:472-520, 835-856, gvrs/GvrsElement.java:298-404.

#include "gvrs_api_internal.h"

struct gf_file {
    GfFileParsed p;
};

namespace {

// what the two reads check of their arguments; fills g, fill and the codec list as the records' calls take it
gf_status fileReadArgs(const gf_context *c, const gf_file *f, const uint8_t *image, size_t imageBytes, bool onDevice, const gf_rect *rect,
                       void *const *blocks, const int32_t *status, GfBlockGeom &g, uint32_t *fill, int *codecs)
{
    if (!c || !f || !image || !rect || !blocks || !status) return GF_ERR_ARG;
    const gf_file_info &i = f->p.info;
    if (onDevice && ((uintptr_t)image & 7) != 0) return GF_ERR_ARG;
    if (imageBytes < i.content_pos) return GF_ERR_ARG;                            // (not the image that was opened)
    for (int k = 0; k < i.n_codecs; k++) codecs[k] = i.codecs[k] == GF_CODEC_UNKNOWN ? GF_CODEC_NONE : i.codecs[k];
    // (the offsets' place is taken by the image: the records' checks only look at it for null)
    const gf_status s = blockReadArgs(c, codecs, i.n_codecs, i.elems, i.n_elems, &i.grid, rect, 0, image, onDevice, (const uint64_t *)image,
                                      blocks, status, g, fill);
    if (s != GF_OK) return s;
    for (int k = 0; k < i.n_codecs; k++)
        if (i.codecs[k] == GF_CODEC_UNKNOWN) return GF_ERR_UNSUPPORTED;
    return GF_OK;
}

}  // namespace

gf_status fileLocateDev(gf_context *c, hipStream_t st, const gf_file_info &i, const uint8_t *dImage, size_t imageBytes, const GfBlockGeom &g,
                        uint8_t *dPresent, GfFileLocateArgs &a)
{
    const size_t T = (size_t)g.nTileRows * (size_t)g.nTileCols;
    Carve k;
    const size_t startsAt = k.add(T * 8), endsAt = k.add(T * 8), verdictAt = k.add(T * 4);
    const gf_status s = c->dFileLoc.ensure(k);
    if (s != GF_OK) return s;
    a = GfFileLocateArgs{dImage, imageBytes, gfFileDirOf(i), g.tileRow0, g.tileCol0, g.nTileRows, g.nTileCols, c->dFileLoc.at<uint64_t>(startsAt),
                         c->dFileLoc.at<uint64_t>(endsAt), c->dFileLoc.at<int32_t>(verdictAt), dPresent};
    GF_HIP(gf_launch_file_locate(a, st));
    return GF_OK;
}

extern "C" {

gf_status gf_file_open(const uint8_t *image, size_t imageBytes, gf_file **out)
{
    if (!image || !out) return GF_ERR_ARG;
    *out = nullptr;
    gf_file *f = new (std::nothrow) gf_file();
    if (!f) return GF_ERR_CAPACITY;
    const gf_status s = gfFileParse(image, imageBytes, f->p);
    if (s != GF_OK) {
        delete f;
        return s;
    }
    *out = f;
    return GF_OK;
}

void gf_file_close(gf_file *f) { delete f; }

gf_status gf_file_get_info(const gf_file *f, gf_file_info *info)
{
    if (!f || !info) return GF_ERR_ARG;
    *info = f->p.info;
    return GF_OK;
}

const char *gf_file_elem_name(const gf_file *f, int e) { return f && e >= 0 && e < f->p.info.n_elems ? f->p.elemNames[e].c_str() : nullptr; }

const char *gf_file_codec_id(const gf_file *f, int k) { return f && k >= 0 && k < f->p.info.n_codecs ? f->p.codecIds[k].c_str() : nullptr; }

const char *gf_file_product_label(const gf_file *f) { return f ? f->p.productLabel.c_str() : nullptr; }

gf_status gf_file_tile_position(const gf_file *f, const uint8_t *image, size_t imageBytes, int32_t tileIndex, uint64_t *pos)
{
    if (!f || !image || !pos) return GF_ERR_ARG;
    *pos = 0;
    if (tileIndex < 0 || tileIndex >= gfTilesOfGrid(f->p.info.grid).count()) return GF_ERR_ARG;
    uint32_t size;
    return gfFileLocate(gfFileDirOf(f->p.info), image, imageBytes, tileIndex, pos, &size);
}

gf_status gf_file_read_block_elems_dev(gf_context *c, const gf_file *f, const uint8_t *dImage, size_t imageBytes,
                                       const gf_rect *rect, int verifyChecksum, void *const *dBlocks, int32_t *dStatus, uint8_t *dPresent)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    int codecs[255];
    gf_status s = fileReadArgs(c, f, dImage, imageBytes, true, rect, dBlocks, dStatus, g, fill, codecs);
    if (s != GF_OK) return s;
    const gf_file_info &i = f->p.info;
    if (!i.checksum_enabled) verifyChecksum = 0;                                  // (the records of such a file carry none: RecordManager.java:492-515)
    const size_t T = (size_t)g.nTileRows * (size_t)g.nTileCols;
    if (T > 0x7fffffffull / (size_t)i.n_elems) return GF_ERR_UNSUPPORTED;         // (as the records' calls: instance numbers travel as 32 bits)
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    GfFileLocateArgs a;
    if ((s = fileLocateDev(c, st, i, dImage, imageBytes, g, dPresent, a)) != GF_OK) return s;
    // the dense list: every slot is a record of the batch, the ones without a record as empty extents whose status k_file_status
    // puts right behind the pipeline -- the host need not know how many tiles are present, and the call synchronises once
    return blockReadDev(c, st, codecs, i.n_codecs, i.elems, i.n_elems, g, fill, T, dImage, imageBytes, a.starts, verifyChecksum, dBlocks,
                        dStatus, a.ends, a.verdict);
}

gf_status gf_file_read_block_elems(gf_context *c, const gf_file *f, const uint8_t *image, size_t imageBytes, const gf_rect *rect,
                                   int verifyChecksum, void *const *blocks, int32_t *status, uint8_t *present)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    int codecs[255];
    gf_status s = fileReadArgs(c, f, image, imageBytes, false, rect, blocks, status, g, fill, codecs);
    if (s != GF_OK) return s;
    const gf_file_info &i = f->p.info;
    if (!i.checksum_enabled) verifyChecksum = 0;
    const size_t T = (size_t)g.nTileRows * (size_t)g.nTileCols, nElems = (size_t)i.n_elems;
    if (T > 0x7fffffffull / nElems) return GF_ERR_UNSUPPORTED;
    // The rectangle's tiles looked up in the host image.  A record the framing walk would refuse for its size word is refused
    // here, so that the staged records are whole, multiples of 8 and end to end.
    std::vector<int32_t> verdict(T);
    std::vector<uint64_t> from, offsets(1, 0);
    gfFileLocateRect(gfFileDirOf(i), image, imageBytes, g.tileRow0, g.tileCol0, g.nTileRows, g.nTileCols, [&](size_t j, int32_t v, uint64_t pos, uint32_t size) {
        if (present) present[j] = pos != 0;
        if (v == GF_OK && pos != 0) {
            if (size < 20u || (size & 7u) != 0u || (uint64_t)size > imageBytes - (pos - 8)) v = GF_ERR_BOUNDS;
            else {
                v = GF_FILE_LOCATED;
                from.push_back(pos - 8);
                offsets.push_back(offsets.back() + size);
            }
        }
        verdict[j] = v;
    });
    const size_t nRec = from.size(), blobBytes = (size_t)offsets.back();
    std::vector<uint8_t> blob(blobBytes + 16);
    for (size_t r = 0; r < nRec; r++) memcpy(blob.data() + offsets[r], image + from[r], (size_t)(offsets[r + 1] - offsets[r]));
    std::vector<int32_t> recStatus(nElems * nRec + 1);
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: the records | offsets | the block of element 0, 1, ... | the records' statuses
    HostStage sg(c);
    int blockP[GF_MAX_ELEMS];
    const int blobP = sg.in(blob.data(), blobBytes, 32), offsetsP = sg.in(offsets.data(), nRec ? (nRec + 1) * 8 : 0);
    stageElems(sg, STAGE_OUT, i.elems, i.n_elems, (size_t)g.nRows * (size_t)g.nCols, blocks, blockP);
    const int statusP = sg.out(recStatus.data(), nElems * nRec * 4);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dBlocks[GF_MAX_ELEMS];
    sg.ptrs(blockP, i.n_elems, dBlocks);
    s = blockReadDev(c, c->stream, codecs, i.n_codecs, i.elems, i.n_elems, g, fill, nRec, sg.ptr<uint8_t>(blobP), blobBytes, sg.ptr<uint64_t>(offsetsP),
                     verifyChecksum, dBlocks, sg.ptr<int32_t>(statusP));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    // the records' statuses to their slots; a tile the file does not hold is GF_OK, a refused entry its verdict
    for (size_t e = 0; e < nElems; e++)
        for (size_t j = 0, r = 0; j < T; j++)
            status[e * T + j] = verdict[j] == GF_FILE_LOCATED ? recStatus[e * nRec + r++] : verdict[j];
    return GF_OK;
}

}  // extern "C"
