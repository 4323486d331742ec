// gvrs_file_emit.h -- a GVRS file image WRITTEN on the host, the counterpart of gvrs_file_parse.h: the file head and header record,
// a metadata record, the metadata directory, the tile directory, the planner of a write and the assembler of a whole image from
// tile records (gf_file_assemble is gfFileAssemble behind the argument checks).  Host arithmetic on bytes: no HIP header, so that
// tests/csrc/file_emit_test.cpp runs it under the sanitizers on any machine.  The device form (gvrs_api_file_write.hip) emits the
// header record, the metadata records and the metadata directory with these functions and shares GF_FILE_CRC_CHUNK with its kernels.
// Reference (core/src/main/java/org/gridfour/): gvrs/GvrsFile.java:239-300, 584-616, gvrs/GvrsFileSpecification.java:1170-1285,
// gvrs/GvrsMetadata.java:217-234, gvrs/RecordManager.java:161-204, 218-219, 670-719, 864-883, 991-1017, :87 and 451-454 (the
// extended directory), gvrs/TileDirectory.java:266-290, gvrs/TileDirectoryExtended.java.  Version 1.04; everything little-endian.
//   a record: [int32 size][type 0 0 0][content][zeros][CRC-32C of the size - 4 bytes in front of it | 0], size = multipleOf8(content + 12)
//   the image: file head | header record | metadata records | tile records | metadata directory | tile directory
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>

#include "gvrs_file_parse.h"

#pragma GCC visibility push(hidden)

// The tile directory's CRC-32C is computed in chunks of this many bytes of the record, on the host and on the device alike (a wave
// per chunk there), and the chunks' checksums are folded in order.  A multiple of 64.
constexpr uint32_t GF_FILE_CRC_CHUNK = 1024;
constexpr uint64_t GF_FILE_MAX_COMPACT_POS = 1ull << 35;         // RecordManager.MAX_NON_EXTENDED_FILE_POS
enum { GF_FILE_REC_METADATA = 1, GF_FILE_REC_TILE = 2, GF_FILE_REC_METADATA_DIR = 4, GF_FILE_REC_TILE_DIR = 5, GF_FILE_REC_HEADER = 6 };
constexpr uint64_t GF_FILE_POS_METADATA_DIR = 64, GF_FILE_POS_TILE_DIR = 80;

// the checksum of p[0, n) as the device computes a tile directory's: chunk by chunk, folded in order (gvrs_crc32c.h)
inline uint32_t gfFileCrc32cChunked(const uint8_t *p, size_t n)
{
    uint32_t crc = 0;                                             // (the checksum of no bytes)
    for (size_t at = 0; at < n; at += GF_FILE_CRC_CHUNK) {
        const size_t len = std::min<size_t>(GF_FILE_CRC_CHUNK, n - at);
        crc = gfCrc32cCombine(crc, gfCrc32c(p + at, len), len);
    }
    return crc;
}

// ---- bytes appended to a vector ----
struct GfFileOut {
    std::vector<uint8_t> &b;
    explicit GfFileOut(std::vector<uint8_t> &v) : b(v) {}
    void le(uint64_t v, int n) { for (int i = 0; i < n; i++) b.push_back((uint8_t)(v >> (8 * i))); }
    void u8(int v) { b.push_back((uint8_t)v); }
    void i16(int v) { le((uint16_t)v, 2); }
    void i32(int32_t v) { le((uint32_t)v, 4); }
    void i64(uint64_t v) { le(v, 8); }
    void f32(float f) { uint32_t u; memcpy(&u, &f, 4); le(u, 4); }
    void f64(double d) { uint64_t u; memcpy(&u, &d, 8); le(u, 8); }
    void zeros(size_t n) { b.insert(b.end(), n, (uint8_t)0); }
    void bytes(const void *p, size_t n) { if (n) b.insert(b.end(), (const uint8_t *)p, (const uint8_t *)p + n); }
    void utf(const char *s) { const size_t n = s ? strlen(s) : 0; le(n, 2); bytes(s, n); }      // (the caller has checked n <= 65535)
    void padTo4() { zeros((4 - (b.size() & 3)) & 3); }
};

inline bool gfFileUtfOk(const char *s) { return !s || strlen(s) <= 65535; }
inline size_t gfFileUtfBytes(const char *s) { return 2 + (s ? strlen(s) : 0); }
GF_HD uint64_t gfFileRecordSize(uint64_t content) { return (content + 12 + 7) & ~7ull; }        // RecordManager.java:219
GF_HD uint64_t gfFileTileDirSize(uint64_t nEntries, bool extended) { return gfFileRecordSize(8 + 16 + nEntries * (extended ? 8 : 4)); }

// the range the header states of an element, and the block write checks cells against: the caller's, or the default constructors'
inline gf_elem_range gfFileElemRange(const gf_elem_spec &s, const gf_file_elem_facts *f)
{
    if (f && f->has_range) return f->range;
    gf_elem_range r;
    r.min_i = s.type == GF_ELEM_SHORT ? -32767 : INT_MIN + 1;
    r.max_i = s.type == GF_ELEM_SHORT ? 32767 : s.type == GF_ELEM_ICF ? INT_MAX - 1 : INT_MAX;
    r.min_f = -INFINITY, r.max_f = INFINITY;
    if (s.type == GF_ELEM_ICF) {                                  // GvrsElementSpecificationIntCodedFloat.java:113-116, in float32
        const float a = (float)r.min_i / s.scale, b = (float)r.max_i / s.scale;
        r.min_f = a + s.offset, r.max_f = b + s.offset;
    }
    return r;
}

// what every call checks of the facts; kinds[n_codecs] (may be null) = the codec list as the record calls take it
inline gf_status gfFileFactsCheck(const gf_file_facts *f, int *kinds)
{
    if (!f || !f->elems || (f->n_codecs > 0 && !f->codec_ids)) return GF_ERR_ARG;
    const gf_grid_spec &g = f->grid;
    if (g.n_rows_grid < 1 || g.n_cols_grid < 1 || g.n_rows_tile < 1 || g.n_cols_tile < 1 || f->n_elems < 1 || f->n_codecs < 0) return GF_ERR_ARG;
    if (!gfFileUtfOk(f->product_label)) return GF_ERR_ARG;
    for (int e = 0; e < f->n_elems && e < GF_MAX_ELEMS; e++) {
        if (f->elems[e].type < GF_ELEM_INT || f->elems[e].type > GF_ELEM_ICF) return GF_ERR_ARG;
        if (f->elem_facts) {
            const gf_file_elem_facts &x = f->elem_facts[e];
            if (!gfFileUtfOk(x.name) || !gfFileUtfOk(x.label) || !gfFileUtfOk(x.description) || !gfFileUtfOk(x.unit)) return GF_ERR_ARG;
        }
    }
    for (int k = 0; k < f->n_codecs && k < 255; k++)
        if (!f->codec_ids[k] || !gfFileUtfOk(f->codec_ids[k])) return GF_ERR_ARG;
    if (f->n_elems > GF_MAX_ELEMS || f->n_codecs > 255) return GF_ERR_UNSUPPORTED;
    for (int k = 0; k < f->n_codecs; k++) {
        const int kind = gfFileCodecKind(f->codec_ids[k]);
        if (kind == GF_CODEC_UNKNOWN) return GF_ERR_UNSUPPORTED;
        if (kinds) kinds[k] = kind;
    }
    if (gfTilesOfGrid(g).count() > 0x7fffffffll) return GF_ERR_UNSUPPORTED;
    return GF_OK;
}

inline gf_status gfFileMetadataCheck(const gf_file_metadata *m, int n)
{
    if (n < 0 || (n > 0 && !m)) return GF_ERR_ARG;
    for (int k = 0; k < n; k++) {
        if (!gfFileUtfOk(m[k].name) || !gfFileUtfOk(m[k].description) || (m[k].content_bytes && !m[k].content)) return GF_ERR_ARG;
        if (m[k].content_bytes > 0x7fffffffull - 65536 * 2 - 64) return GF_ERR_ARG;           // (the record's size is an int32)
    }
    return GF_OK;
}

// The bytes [0, content_pos) of a file: the file head and the header record, with the two directory positions as given.  finished:
// with the record's checksum where checksums are on (the device form patches the positions and computes it afterwards).  The facts
// have passed gfFileFactsCheck.
inline void gfFileEmitHeader(const gf_file_facts &f, uint64_t metadataDirPos, uint64_t tileDirPos, bool finished, std::vector<uint8_t> &out)
{
    out.clear();
    GfFileOut o(out);
    o.bytes("gvrs raster\0", 12);
    o.u8(1), o.u8(4), o.u8(0), o.u8(0);
    o.i32(0);                                                     // the record's size: below
    o.u8(GF_FILE_REC_HEADER), o.zeros(3);
    o.bytes(f.uuid, 16);
    o.i64((uint64_t)f.time_modified);
    o.i64(0);                                                     // opened for writing
    o.i64(0);                                                     // no free-space directory
    o.i64(metadataDirPos);
    o.i16(1), o.zeros(6);                                         // levels
    o.i64(tileDirPos);
    o.zeros(16);
    // the specification (GvrsFileSpecification.write)
    o.i32(f.grid.n_rows_grid), o.i32(f.grid.n_cols_grid), o.i32(f.grid.n_rows_tile), o.i32(f.grid.n_cols_tile);
    o.zeros(8);
    o.u8(f.checksum_enabled ? 1 : 0), o.u8(f.raster_space), o.u8(f.coordinate_system), o.zeros(5);
    o.f64(f.x0), o.f64(f.y0), o.f64(f.x1), o.f64(f.y1), o.f64(f.cell_size_x), o.f64(f.cell_size_y);
    for (const double v : f.m2r) o.f64(v);
    for (const double v : f.r2m) o.f64(v);
    o.i32(f.n_elems);
    for (int e = 0; e < f.n_elems; e++) {
        const gf_elem_spec &s = f.elems[e];
        const gf_file_elem_facts *x = f.elem_facts ? &f.elem_facts[e] : nullptr;
        const gf_elem_range r = gfFileElemRange(s, x);
        static const int code[4] = {0, 3, 2, 1};                  // GvrsElementType's code values of GF_ELEM_INT, SHORT, FLOAT, ICF
        char generic[16];
        snprintf(generic, sizeof(generic), "e%d", e);
        o.u8(code[s.type]), o.u8(x && x->continuous ? 1 : 0), o.zeros(6);
        o.utf(x && x->name ? x->name : x ? "" : generic);
        o.padTo4();
        switch (s.type) {
        case GF_ELEM_SHORT: o.i16(r.min_i), o.i16(r.max_i), o.i16(s.fill_i); break;
        case GF_ELEM_FLOAT: o.f32(r.min_f), o.f32(r.max_f), o.f32(s.fill_f); break;
        case GF_ELEM_ICF:
            o.f32(r.min_f), o.f32(r.max_f), o.f32(s.fill_f), o.f32(s.scale), o.f32(s.offset);
            o.i32(r.min_i), o.i32(r.max_i), o.i32(s.fill_i);
            break;
        default: o.i32(r.min_i), o.i32(r.max_i), o.i32(s.fill_i); break;
        }
        o.utf(x ? x->label : nullptr), o.utf(x ? x->description : nullptr), o.utf(x ? x->unit : nullptr);
        o.padTo4();
    }
    o.i32(f.n_codecs);
    for (int k = 0; k < f.n_codecs; k++) o.utf(f.codec_ids[k]);
    o.utf(f.product_label);
    // 8 reserved bytes, the checksum word, padding to a multiple of 8 of the file position (GvrsFile.java:274-290)
    const size_t contentPos = (out.size() + 8 + 4 + 7) & ~(size_t)7, size = contentPos - 16;
    o.zeros(contentPos - out.size());
    gfPutLe(&out[16], size, 4);
    if (finished && f.checksum_enabled) gfPutLe(&out[contentPos - 4], gfCrc32c(out.data() + 16, size - 4), 4);
}

// a record's frame around content that begins at out[start + 8] and ends at out's end: size and type words, padding, checksum.
// size: the record's, where it is given (at least the content's need); else the smallest that holds the content
inline void gfFileCloseRecord(std::vector<uint8_t> &out, size_t start, int type, bool checksums, bool chunked = false, size_t size = 0)
{
    if (size == 0) size = (size_t)gfFileRecordSize(out.size() - start - 8);
    out.resize(start + size, 0);
    gfPutLe(&out[start], size, 4);
    gfPutLe(&out[start + 4], (uint64_t)type, 4);
    if (checksums) gfPutLe(&out[start + size - 4], chunked ? gfFileCrc32cChunked(out.data() + start, size - 4) : gfCrc32c(out.data() + start, size - 4), 4);
}

// one metadata record appended (GvrsMetadata.write in RecordManager.writeMetadata's frame); returns its content position in out
inline size_t gfFileEmitMetadata(const gf_file_metadata &m, bool checksums, std::vector<uint8_t> &out)
{
    const size_t start = out.size();
    GfFileOut o(out);
    o.zeros(8);
    o.utf(m.name);
    o.i32(m.record_id);
    o.u8(m.type), o.zeros(3);
    o.i32((int32_t)m.content_bytes);
    o.bytes(m.content, (size_t)m.content_bytes);
    o.utf(m.description);
    gfFileCloseRecord(out, start, GF_FILE_REC_METADATA, checksums);
    return start + 8;
}

// the metadata directory appended: positions[k] = the content position of record k in the file, ascending
inline void gfFileEmitMetadataDir(const gf_file_metadata *m, const uint64_t *positions, int n, bool checksums, std::vector<uint8_t> &out)
{
    if (n == 0) return;
    const size_t start = out.size();
    GfFileOut o(out);
    o.zeros(8);
    o.i32(n);
    for (int k = 0; k < n; k++) {
        o.i64(positions[k]);
        o.utf(m[k].name);
        o.i32(m[k].record_id);
        o.u8(m[k].type);
    }
    gfFileCloseRecord(out, start, GF_FILE_REC_METADATA_DIR, checksums);
}

// the tile directory appended: positions[nRows * nCols] = the content position of each tile's record, or 0, row-major
inline void gfFileEmitTileDir(bool extended, int32_t row0, int32_t col0, int32_t nRows, int32_t nCols, const uint64_t *positions, bool checksums,
                              std::vector<uint8_t> &out)
{
    const size_t start = out.size(), n = (size_t)nRows * (size_t)nCols;
    GfFileOut o(out);
    o.zeros(8);
    o.u8(0), o.u8(extended ? 1 : 0), o.zeros(6);
    o.i32(row0), o.i32(col0), o.i32(nRows), o.i32(nCols);
    for (size_t k = 0; k < n; k++) {
        if (extended) o.i64(positions[k]);
        else o.le(positions[k] / 8, 4);
    }
    gfFileCloseRecord(out, start, GF_FILE_REC_TILE_DIR, checksums, true);
}

// What a write lays in front of the tile records, and what it knows of the metadata directory before it knows where it goes (the
// metadata records lie in front of the tile records, so their positions are final): front = head | header record (positions 0, no
// checksum unless finished later) | metadata records; metaDir = the whole directory record.
struct GfFileFront {
    std::vector<uint8_t> front, metaDir;
    uint64_t contentPos = 0;                  // the header record's end
    uint64_t firstRecordPos() const { return front.size(); }
};

inline void gfFileEmitFront(const gf_file_facts &f, const gf_file_metadata *m, int nMeta, GfFileFront &w)
{
    gfFileEmitHeader(f, 0, 0, false, w.front);
    w.contentPos = w.front.size();
    std::vector<uint64_t> positions((size_t)nMeta);
    for (int k = 0; k < nMeta; k++) positions[(size_t)k] = gfFileEmitMetadata(m[k], f.checksum_enabled != 0, w.front);
    w.metaDir.clear();
    gfFileEmitMetadataDir(m, positions.data(), nMeta, f.checksum_enabled != 0, w.metaDir);
}

// the header record of front finished in place: the two positions and, where checksums are on, the record's checksum
inline void gfFileFinishHeader(std::vector<uint8_t> &front, uint64_t contentPos, uint64_t metadataDirPos, uint64_t tileDirPos, bool checksums)
{
    gfPutLe(&front[GF_FILE_POS_METADATA_DIR], metadataDirPos, 8);
    gfPutLe(&front[GF_FILE_POS_TILE_DIR], tileDirPos, 8);
    if (checksums) gfPutLe(&front[contentPos - 4], gfCrc32c(front.data() + 16, (size_t)contentPos - 16 - 4), 4);
}

// gf_file_write_plan behind its argument checks: the tiles a write covers (nOut) -> the first record's position and the largest image
inline void gfFilePlan(const GfFileFront &w, uint64_t nOut, uint64_t maxRecordBytes, int flags, uint64_t *firstRecordPos, uint64_t *maxImageBytes)
{
    const uint64_t p0 = w.firstRecordPos(), recordsEnd = p0 + nOut * maxRecordBytes;
    const bool extended = (flags & GF_FILE_DIR_EXTENDED) != 0 || recordsEnd > GF_FILE_MAX_COMPACT_POS;
    if (firstRecordPos) *firstRecordPos = p0;
    if (maxImageBytes) *maxImageBytes = recordsEnd + w.metaDir.size() + gfFileTileDirSize(nOut, extended);
}

// gf_file_assemble behind the checks of facts and metadata (gvrs_hip_codec.h has the contract)
inline gf_status gfFileAssemble(const gf_file_facts &f, const gf_file_metadata *m, int nMeta, int flags, const uint8_t *blob, const uint64_t *offsets,
                                const int32_t *tileIndices, size_t nRecords, uint8_t *image, size_t imageCap, uint64_t *imageBytes)
{
    if (!imageBytes || (nRecords && (!offsets || !tileIndices)) || (!image && imageCap)) return GF_ERR_ARG;
    *imageBytes = 0;
    const gf_grid_spec &g = f.grid;
    const int64_t nColsOfTiles = gfTilesOfGrid(g).cols, nTiles = gfTilesOfGrid(g).count();
    GfFileFront w;
    gfFileEmitFront(f, m, nMeta, w);
    // the records' places, the bounding rectangle of their tiles and the extended decision
    struct Placed { int32_t tile; uint64_t pos; };
    std::vector<Placed> placed;
    uint64_t at = w.firstRecordPos();
    int64_t r0 = INT_MAX, r1 = -1, c0 = INT_MAX, c1 = -1;
    bool extended = (flags & GF_FILE_DIR_EXTENDED) != 0;
    for (size_t r = 0; r < nRecords; r++) {
        if (offsets[r + 1] < offsets[r] || tileIndices[r] < 0 || tileIndices[r] >= nTiles) return GF_ERR_ARG;
        const uint64_t len = offsets[r + 1] - offsets[r];
        if (len == 0) continue;
        if ((len & 7) != 0 || len < 24) return GF_ERR_ARG;
        const int64_t tr = tileIndices[r] / nColsOfTiles, tc = tileIndices[r] % nColsOfTiles;
        r0 = std::min(r0, tr), r1 = std::max(r1, tr), c0 = std::min(c0, tc), c1 = std::max(c1, tc);
        placed.push_back(Placed{tileIndices[r], at + 8});
        extended |= at + 8 > GF_FILE_MAX_COMPACT_POS;
        at += len;
    }
    std::vector<Placed> byTile(placed);
    std::sort(byTile.begin(), byTile.end(), [](const Placed &a, const Placed &b) { return a.tile < b.tile; });
    for (size_t k = 1; k < byTile.size(); k++)
        if (byTile[k].tile == byTile[k - 1].tile) return GF_ERR_ARG;
    const uint64_t recordsEnd = at;
    const int32_t nRows = placed.empty() ? 0 : (int32_t)(r1 - r0 + 1), nCols = placed.empty() ? 0 : (int32_t)(c1 - c0 + 1);
    if (placed.empty()) r0 = c0 = 0;
    const uint64_t nEntries = (uint64_t)nRows * (uint64_t)nCols;
    const uint64_t total = recordsEnd + w.metaDir.size() + gfFileTileDirSize(nEntries, extended);
    *imageBytes = total;
    if (total > imageCap) return GF_ERR_CAPACITY;
    if (!blob && !placed.empty()) return GF_ERR_ARG;
    std::vector<uint64_t> positions((size_t)nEntries, 0);
    for (const Placed &p : placed) positions[(size_t)((p.tile / nColsOfTiles - r0) * nCols + (p.tile % nColsOfTiles - c0))] = p.pos;
    std::vector<uint8_t> tileDir;
    gfFileEmitTileDir(extended, (int32_t)r0, (int32_t)c0, nRows, nCols, positions.data(), f.checksum_enabled != 0, tileDir);
    gfFileFinishHeader(w.front, w.contentPos, w.metaDir.empty() ? 0 : recordsEnd + 8, recordsEnd + w.metaDir.size() + 8, f.checksum_enabled != 0);
    memcpy(image, w.front.data(), w.front.size());
    at = w.firstRecordPos();
    for (size_t r = 0; r < nRecords; r++) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        if (len) memmove(image + at, blob + offsets[r], len);              // (gf_file_write_block_elems: the records may lie there already)
        at += len;
    }
    if (!w.metaDir.empty()) memcpy(image + recordsEnd, w.metaDir.data(), w.metaDir.size());
    memcpy(image + recordsEnd + w.metaDir.size(), tileDir.data(), tileDir.size());
    return GF_OK;
}

#pragma GCC visibility pop
