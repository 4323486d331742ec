// gvrs_api_records_enc.hip -- tile records of several elements WRITTEN: gf_tile_record_encode_batch_elems_dev frames and checksums in
// device memory what the codecs' device encoders left in their slots (kernels: gvrs_records_enc.hip), gf_tile_record_encode_batch_elems
// is the same call for host memory and, for codec lists that need the host's zlib, the element-by-element generalisation of
// gf_tile_record_encode_batch.
// Reference: gvrs/RecordManager.java:386-490 (writeTile), gvrs/RasterTile.java:234-256 (getCompressedPacking), TileElement{Int,Short,
// Float,IntCodedFloat}.encode, gvrs/CodecMaster.java:150-169 (encode), 261-280 (encodeFloats).

#include "gvrs_api_internal.h"

namespace {

bool isIntElem(int type) { return type != GF_ELEM_FLOAT; }

}  // namespace

// what the host can check without a device; values / blob / offsets: device or host pointers, only looked at for null and alignment
gf_status encArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                  size_t nTiles, const int32_t *tileIndices, const void *const *values, const uint8_t *blob, size_t blobCap,
                  const uint64_t *offsets, bool onDevice, const int32_t *dStatus)
{
    if (!c || !elems || !tileIndices || !values || !offsets || (!blob && blobCap) || (!codecs && nCodecs > 0)) return GF_ERR_ARG;
    if (onDevice && (!blob || !dStatus || ((uintptr_t)blob & 7) != 0)) return GF_ERR_ARG;
    if (nElems < 1 || nElems > GF_MAX_ELEMS || nRows < 1 || nCols < 1 || nCodecs > 255) return GF_ERR_ARG;
    for (int e = 0; e < nElems; e++) {
        if (!values[e] || elems[e].type < GF_ELEM_INT || elems[e].type > GF_ELEM_ICF) return GF_ERR_ARG;
        if (elems[e].type == GF_ELEM_ICF && (elems[e].scale == 0.0f || std::isnan(elems[e].scale))) return GF_ERR_ARG;
        if (elems[e].type == GF_ELEM_SHORT && (elems[e].fill_i < -32768 || elems[e].fill_i > 32767)) return GF_ERR_ARG;
        if (onDevice && ((uintptr_t)values[e] & 3) != 0) return GF_ERR_ARG;
    }
    for (int k = 0; k < nCodecs; k++)
        if (codecs[k] < GF_CODEC_NONE || codecs[k] > GF_CODEC_LSOP08) return GF_ERR_ARG;
    if (nTiles > 0x7fffffffull / (size_t)nElems) return GF_ERR_UNSUPPORTED;         // instance numbers travel as 32 bits
    if ((size_t)nRows * (size_t)nCols >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    if (gf_tile_record_max_bytes_elems(elems, nElems, nRows, nCols) > 0x7fffffffull) return GF_ERR_UNSUPPORTED;   // the size field is an int32
    return GF_OK;
}

// the lists whose records need nothing from the host: CodecHuffman / CodecCanonHuffman entries, and entries without an integer codec
// as long as no element would go to the CodecFloat that stands there
bool deviceList(const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems)
{
    bool anyFloat = false;
    for (int e = 0; e < nElems; e++) anyFloat |= elems[e].type == GF_ELEM_FLOAT;
    for (int k = 0; k < nCodecs; k++) {
        if (codecs[k] == GF_CODEC_DEFLATE || codecs[k] == GF_CODEC_LSOP12 || codecs[k] == GF_CODEC_LSOP08) return false;
        if (codecs[k] == GF_CODEC_NONE && anyFloat) return false;
    }
    return true;
}

// the one device pipeline (no lock taken, no argument checked).  Enqueues only: every codec runs on every tile and the layout is a
// scan, so nothing has to come back to the host.  dPreStatus (may be null), per tile: a non-zero entry is the tile's status and the
// tile gets no record (k_record_plan); the encoders run on such a tile all the same.
gf_status recordsEncodeDev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows,
                           int nCols, size_t nTiles, const int32_t *dTileIndices, const void *const *dValues, int checksumEnabled,
                           uint8_t *dBlob, size_t blobCap, uint64_t *dOffsets, uint8_t *dCodecUsed, int32_t *dStatus,
                           const int32_t *dPreStatus)
{
    if (nCodecs < 0) nCodecs = 0;
    const size_t cells = (size_t)nRows * (size_t)nCols, n = nTiles, nInst = (size_t)nElems * n;
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = streamOf(c, stream);
    GfRecordPlanArgs p{};
    int act[256], nAct = 0;
    for (int k = 0; k < nCodecs; k++)
        if (codecs[k] == GF_CODEC_HUFFMAN || codecs[k] == GF_CODEC_CANON_HUFFMAN) {
            p.actIndex[nAct] = (uint8_t)k;
            act[nAct++] = k;
        }
    // sizes of the temporaries ("records written on the device")
    Carve slots, wide, meta;
    size_t nCandArrays = 0, slotAt[GF_MAX_ELEMS] = {}, wideAt[GF_MAX_ELEMS] = {};
    for (int e = 0; e < nElems; e++) {
        const size_t stdSize = elemStandardSize(elems[e].type == GF_ELEM_SHORT ? GF_ELEM_SHORT : GF_ELEM_INT, cells);
        p.elems[e].values = dValues[e];
        p.elems[e].stdSize = (uint32_t)stdSize;
        p.elems[e].srcBytes = (uint32_t)(cells * elemItemBytes(elems[e].type));
        if (isIntElem(elems[e].type) && nAct > 0) {
            p.elems[e].slotStride = (uint32_t)roundUp(stdSize, 16);
            p.elems[e].cand0 = (uint32_t)nCandArrays;
            slotAt[e] = slots.add((size_t)nAct * n * p.elems[e].slotStride);
            nCandArrays += (size_t)nAct;
            if (elems[e].type == GF_ELEM_SHORT) wideAt[e] = wide.add(n * cells * 4);
        }
    }
    // per candidate length and status; per instance (a multiple of 16 of them) length and position; per record its size; per instance its source
    const size_t nCand = nCandArrays * n, instPad = roundUp(nInst, 16);
    const size_t candLenAt = meta.add(nCand * 4), candStatusAt = meta.add(nCand * 4), elemLenAt = meta.add(instPad * 4), elemPosAt = meta.add(instPad * 4);
    const size_t sizesAt = meta.add(n * 4), elemSrcAt = meta.add(instPad);
    gf_status s;
    if ((s = c->dEncMeta.ensure(meta, 64)) != GF_OK) return s;
    if (slots.total && (s = c->dEncSlots.ensure(slots)) != GF_OK) return s;
    if (wide.total && (s = c->dEncWide.ensure(wide)) != GF_OK) return s;
    const DevBuf &m = c->dEncMeta;
    uint32_t *candLen = m.at<uint32_t>(candLenAt), *elemLen = m.at<uint32_t>(elemLenAt), *elemPos = m.at<uint32_t>(elemPosAt), *sizes = m.at<uint32_t>(sizesAt);
    int32_t *candStatus = m.at<int32_t>(candStatusAt);
    uint8_t *elemSrc = m.at<uint8_t>(elemSrcAt);

    // the codecs: every integer codec of the list on every integer element, in element order, then list order
    for (int e = 0; e < nElems; e++) {
        if (!p.elems[e].slotStride) continue;
        p.elems[e].slots = c->dEncSlots.at<const uint8_t>(slotAt[e]);
        const int32_t *iv = (const int32_t *)dValues[e];                            // INT, and the codes of an ICF element, in place
        if (elems[e].type == GF_ELEM_SHORT) {
            int32_t *widened = c->dEncWide.at<int32_t>(wideAt[e]);
            GF_HIP(gf_launch_elem_widen((const int16_t *)dValues[e], widened, n * cells, elems[e].fill_i, st));
            iv = widened;
        }
        for (int a = 0; a < nAct; a++) {
            const size_t cand = ((size_t)p.elems[e].cand0 + a) * n;
            uint8_t *slotsOf = c->dEncSlots.at<uint8_t>(slotAt[e] + (size_t)a * n * p.elems[e].slotStride);
            s = encodeBatchDev(codecs[act[a]] == GF_CODEC_HUFFMAN ? KIND_HUFFMAN : KIND_CANON, c, st, act[a], nRows, nCols, n, iv, slotsOf,
                               p.elems[e].slotStride, candLen + cand, nullptr, candStatus + cand, GF_PM_ALL, 0);
            if (s != GF_OK) return s;
        }
    }
    p.nTiles = n;
    p.nElems = nElems;
    p.nAct = nAct;
    p.candLen = candLen;
    p.candStatus = candStatus;
    p.elemLen = elemLen;
    p.elemPos = elemPos;
    p.elemSrc = elemSrc;
    p.sizes = sizes;
    p.status = dStatus;
    p.codecUsed = dCodecUsed;
    p.preStatus = dPreStatus;
    GF_HIP(gf_launch_record_plan(p, st));
    GF_HIP(gf_launch_record_scan(sizes, dOffsets, n, st));
    GfRecordWriteArgs w{};
    w.nTiles = n;
    w.nElems = nElems;
    w.checksum = checksumEnabled ? 1 : 0;
    w.tileIndices = dTileIndices;
    w.elemLen = elemLen;
    w.elemPos = elemPos;
    w.elemSrc = elemSrc;
    w.sizes = sizes;
    w.offsets = dOffsets;
    w.blob = dBlob;
    w.blobCap = blobCap;
    memcpy(w.elems, p.elems, sizeof w.elems);
    GF_HIP(gf_launch_record_write(w, st));
    if (checksumEnabled) GF_HIP(gf_launch_record_crc32c_write(dBlob, blobCap, dOffsets, sizes, n, st));
    return GF_OK;
}

// a list with CodecDeflate, LSOP12 or CodecFloat at work: element by element through the host entry points, framed on host threads
// (the loop of gf_tile_record_encode_batch over the elements of a tile)
gf_status recordsEncodeHost(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows, int nCols,
                            size_t nTiles, const int32_t *tileIndices, const void *const *values, int checksumEnabled, uint8_t *blob,
                            size_t blobCap, uint64_t *offsets, uint8_t *codecUsed)
{
    const size_t cells = (size_t)nRows * (size_t)nCols;
    struct Elem {
        std::vector<uint8_t> packs;
        std::vector<uint64_t> off;
        std::vector<uint8_t> used;
        std::vector<uint32_t> len;
        size_t stdSize = 0;
    };
    std::vector<Elem> el(nElems);
    bool anyInt = false;
    int floatSlot = -1;
    for (int k = 0; k < nCodecs; k++) {
        if (codecs[k] != GF_CODEC_NONE) anyInt = true;
        else if (floatSlot < 0) floatSlot = k;
    }
    for (int e = 0; e < nElems; e++) {
        Elem &x = el[e];
        const int type = elems[e].type;
        x.stdSize = elemStandardSize(type == GF_ELEM_SHORT ? GF_ELEM_SHORT : GF_ELEM_INT, cells);
        x.off.assign(nTiles + 1, 0);
        x.used.assign(nTiles, 0xff);
        x.len.assign(nTiles, (uint32_t)x.stdSize);
        std::vector<int32_t> st(nTiles, GF_DECLINED);
        gf_status s = GF_OK;
        if (type == GF_ELEM_FLOAT) {
            if (floatSlot < 0) continue;                                         // CodecMaster.encodeFloats finds no codec: null
            x.packs.resize(nTiles * (cells * 5 + 1024) + 64);
            // (level 6: what the reference's sample files were written with, see gf_float_encode_batch_f32)
            s = gf_float_encode_batch_f32(c, floatSlot, nRows, nCols, nTiles, (const float *)values[e], 6, x.packs.data(), x.packs.size(), x.off.data());
            if (s == GF_ERR_CAPACITY) {
                x.packs.resize((size_t)x.off[nTiles] + 64);
                s = gf_float_encode_batch_f32(c, floatSlot, nRows, nCols, nTiles, (const float *)values[e], 6, x.packs.data(), x.packs.size(), x.off.data());
            }
            if (s != GF_OK) return s;
            for (size_t t = 0; t < nTiles; t++) {
                st[t] = x.off[t + 1] > x.off[t] ? GF_OK : GF_DECLINED;
                x.used[t] = (uint8_t)floatSlot;
            }
        } else {
            if (!anyInt) continue;
            const int32_t *iv = (const int32_t *)values[e];
            std::vector<int32_t> widened;
            if (type == GF_ELEM_SHORT) {
                const int16_t *sv = (const int16_t *)values[e];
                const int16_t fill = (int16_t)elems[e].fill_i;
                widened.resize(nTiles * cells);
                parallelFor(nTiles, [&](size_t t) {
                    for (size_t i = t * cells; i < (t + 1) * cells; i++) widened[i] = sv[i] == fill ? (int32_t)0x80000000 : (int32_t)sv[i];
                });
                iv = widened.data();
            }
            x.packs.resize(nTiles * (cells * 4 + 1024) + 64);
            s = gf_codec_master_encode_batch_i32(c, codecs, nCodecs, nRows, nCols, nTiles, iv, x.packs.data(), x.packs.size(), x.off.data(),
                                                 x.used.data(), st.data());
            if (s == GF_ERR_CAPACITY) {
                x.packs.resize((size_t)x.off[nTiles] + 64);
                s = gf_codec_master_encode_batch_i32(c, codecs, nCodecs, nRows, nCols, nTiles, iv, x.packs.data(), x.packs.size(), x.off.data(),
                                                     x.used.data(), st.data());
            }
            if (s != GF_OK) return s;
        }
        for (size_t t = 0; t < nTiles; t++) {
            if (st[t] < 0) return (gf_status)st[t];                              // an encoder threw: the Java call fails as a whole
            const size_t len = st[t] == GF_OK ? (size_t)(x.off[t + 1] - x.off[t]) : 0;
            if (st[t] != GF_OK || len == 0 || len >= x.stdSize) x.used[t] = 0xff;
            else x.len[t] = (uint32_t)len;
        }
    }
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        uint64_t content = 4;
        for (int e = 0; e < nElems; e++) content += 4 + (uint64_t)el[e].len[t];
        offsets[t] = total;
        total += (content + 12 + 7) & ~(uint64_t)7;                              // multipleOf8(content + RECORD_OVERHEAD_SIZE)
    }
    offsets[nTiles] = total;
    if (codecUsed)
        for (int e = 0; e < nElems; e++) memcpy(codecUsed + (size_t)e * nTiles, el[e].used.data(), nTiles);
    if (total > blobCap) return GF_ERR_CAPACITY;
    parallelFor(nTiles, [&](size_t t) {
        uint8_t *r = blob + offsets[t];
        const size_t size = (size_t)(offsets[t + 1] - offsets[t]);
        memset(r, 0, size);
        putLE32(r, (uint32_t)size);
        r[4] = 2;                                                                // RecordType.Tile
        putLE32(r + 8, (uint32_t)tileIndices[t]);
        size_t pos = 12;
        for (int e = 0; e < nElems; e++) {
            const Elem &x = el[e];
            putLE32(r + pos, x.len[t]);
            if (x.used[t] != 0xff) memcpy(r + pos + 4, x.packs.data() + x.off[t], x.len[t]);
            else memcpy(r + pos + 4, (const uint8_t *)values[e] + t * cells * elemItemBytes(elems[e].type), cells * elemItemBytes(elems[e].type));
            pos += 4 + x.len[t];
        }
        if (checksumEnabled) putLE32(r + size - 4, gf_crc32c(r, size - 4));
    });
    return GF_OK;
}

extern "C" {

size_t gf_tile_record_max_bytes_elems(const gf_elem_spec *elems, int nElems, int nRows, int nCols)
{
    if (!elems || nElems < 1 || nElems > GF_MAX_ELEMS || nRows < 1 || nCols < 1) return 0;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    size_t content = 4;
    for (int e = 0; e < nElems; e++) content += 4 + elemStandardSize(elems[e].type == GF_ELEM_SHORT ? GF_ELEM_SHORT : GF_ELEM_INT, cells);
    return (content + 12 + 7) & ~(size_t)7;
}

gf_status gf_tile_record_encode_batch_elems_dev(gf_context *c, void *stream, const int *codecs, int nCodecs, const gf_elem_spec *elems,
                                                int nElems, int nRows, int nCols, size_t nTiles, const int32_t *dTileIndices,
                                                const void *const *dValues, int checksumEnabled, uint8_t *dBlob, size_t blobCap,
                                                uint64_t *dOffsets, uint8_t *dCodecUsed, int32_t *dStatus)
{
    gf_status s = encArgs(c, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, dTileIndices, dValues, dBlob, blobCap, dOffsets, true, dStatus);
    if (s != GF_OK) return s;
    if (!deviceList(codecs, nCodecs, elems, nElems)) return GF_ERR_UNSUPPORTED;
    if (nTiles == 0) return GF_OK;
    GF_CTX_LOCK(c);
    return recordsEncodeDev(c, stream, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, dTileIndices, dValues, checksumEnabled, dBlob,
                            blobCap, dOffsets, dCodecUsed, dStatus);
}

gf_status gf_tile_record_encode_batch_elems(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, int nRows,
                                            int nCols, size_t nTiles, const int32_t *tileIndices, const void *const *values,
                                            int checksumEnabled, uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *codecUsed)
{
    gf_status s = encArgs(c, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, tileIndices, values, blob, blobCap, offsets, false, nullptr);
    if (s != GF_OK) return s;
    if (nTiles == 0) {
        offsets[0] = 0;
        return GF_OK;
    }
    GF_CTX_LOCK(c);
    if (nCodecs < 0) nCodecs = 0;
    if (!deviceList(codecs, nCodecs, elems, nElems))
        return recordsEncodeHost(c, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, tileIndices, values, checksumEnabled, blob, blobCap,
                                 offsets, codecUsed);
    // staged and sent through the device form: values of element 0, 1, ... (four spare bytes behind each) | tile indices | the blob at
    // its largest | offsets | statuses | codec_used; the offsets say how much of the blob counts
    GF_HIP(hipSetDevice(c->device));
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t maxBlob = nTiles * gf_tile_record_max_bytes_elems(elems, nElems, nRows, nCols);
    std::vector<int32_t> status(nTiles);
    HostStage sg(c);
    int valueP[GF_MAX_ELEMS];
    stageElems(sg, STAGE_IN, elems, nElems, nTiles * cells, values, valueP, 4);
    const int indicesP = sg.in(tileIndices, nTiles * 4), blobP = sg.held(blob, maxBlob), offsetsP = sg.out(offsets, (nTiles + 1) * 8);
    const int statusP = sg.out(status.data(), nTiles * 4), usedP = sg.out(codecUsed, (size_t)nElems * nTiles);
    if ((s = sg.begin()) != GF_OK) return s;
    void *dValues[GF_MAX_ELEMS];
    sg.ptrs(valueP, nElems, dValues);
    s = recordsEncodeDev(c, c->stream, codecs, nCodecs, elems, nElems, nRows, nCols, nTiles, sg.ptr<int32_t>(indicesP), dValues, checksumEnabled,
                         sg.ptr<uint8_t>(blobP), maxBlob, sg.ptr<uint64_t>(offsetsP), sg.ptr<uint8_t>(usedP), sg.ptr<int32_t>(statusP));
    if (s != GF_OK || (s = sg.flush()) != GF_OK) return s;
    for (size_t t = 0; t < nTiles; t++)
        if (status[t] < 0) return (gf_status)status[t];                          // an encoder threw: the Java call fails as a whole
    if (offsets[nTiles] > blobCap) return GF_ERR_CAPACITY;
    return (s = sg.fetch(blobP, (size_t)offsets[nTiles])) != GF_OK ? s : sg.end();
}

}  // extern "C"
