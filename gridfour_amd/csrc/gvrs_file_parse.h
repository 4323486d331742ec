// gvrs_file_parse.h -- a GVRS file image read on the host: the file head, the header record with its specification of grid, tiles,
// elements and codec list, the 24-byte prefix of the tile directory, and one tile's directory entry with its record head.  Host
// arithmetic on bytes: no HIP header, so that tests/csrc/file_parse_test.cpp runs it under the sanitizers on any machine.  Every
// read is checked against the image's length first; nothing here keeps a pointer into the image.
// Reference (core/src/main/java/org/gridfour/): gvrs/GvrsFile.java:341-483, gvrs/GvrsFileSpecification.java:856-1052, 1154-1160,
// gvrs/RecordManager.java:835-856, gvrs/TileDirectory.java:200-257, gvrs/TileDirectoryExtended.java, io/BufferedRandomAccessFile
// leReadUTF.  Version 1.04; everything little-endian.
//   bytes 0..11 "gvrs raster\0", 12 version, 13 sub-version, 2 reserved
//   16 int32 header-record size (content starts at 16 + size; CRC-32C of [16, 16 + size - 4) in its last 4 bytes), 20 record type + 3,
//   24 UUID, 40 time modified, 48 time opened for writing, 56 free-space directory, 64 metadata directory, 72 int16 levels + 6,
//   80 tile directory, 16 reserved, 104 the specification
//   tile directory at P: byte P + 1 the extended flag, 8 bytes of prefix, int32 row0 col0 nRows nCols, then nRows * nCols entries
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gvrs_hip_codec.h"
#include "gvrs_crc32c.h"

#pragma GCC visibility push(hidden)          // nothing here is an export of the library

constexpr uint64_t GF_FILE_SPEC_POS = 104, GF_FILE_DIR_PREFIX = 24;

struct GfFileParsed {
    gf_file_info info;
    std::vector<std::string> elemNames, codecIds;
    std::string productLabel;
};

// little-endian get and put of n bytes, for every header of the chain
GF_HD uint64_t gfLe(const uint8_t *p, int n)
{
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
GF_HD void gfPutLe(uint8_t *p, uint64_t v, int n) { for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i)); }

// the tile rows and tile columns of a grid
struct GfTilesOfGrid {
    int64_t rows, cols;
    int64_t count() const { return rows * cols; }
};
inline GfTilesOfGrid gfTilesOfGrid(const gf_grid_spec &g)
{
    return GfTilesOfGrid{((int64_t)g.n_rows_grid + g.n_rows_tile - 1) / g.n_rows_tile, ((int64_t)g.n_cols_grid + g.n_cols_tile - 1) / g.n_cols_tile};
}

// A cursor over image[0, limit), limit <= bytes.  A read that would pass the limit fails the cursor: GF_ERR_BOUNDS where the image
// itself ends there (a truncated image), GF_ERR_FORMAT where the header record does.  A failed cursor reads zeros.
struct GfFileCursor {
    const uint8_t *image;
    uint64_t bytes, limit, pos;
    gf_status status = GF_OK;
    GfFileCursor(const uint8_t *im, uint64_t n, uint64_t lim, uint64_t at) : image(im), bytes(n), limit(lim < n ? lim : n), pos(at) {}
    bool need(uint64_t n)
    {
        if (status != GF_OK) return false;
        if (pos > limit || n > limit - pos) {
            status = limit == bytes ? GF_ERR_BOUNDS : GF_ERR_FORMAT;
            return false;
        }
        return true;
    }
    void skip(uint64_t n) { if (need(n)) pos += n; }
    void alignTo4() { skip((4 - (pos & 3)) & 3); }             // (a multiple of 4 of the FILE position)
    uint64_t le(int n)
    {
        if (!need((uint64_t)n)) return 0;
        pos += (uint64_t)n;
        return gfLe(image + pos - n, n);
    }
    uint8_t u8() { return (uint8_t)le(1); }
    int16_t i16() { return (int16_t)(uint16_t)le(2); }
    int32_t i32() { return (int32_t)(uint32_t)le(4); }
    uint64_t u64() { return le(8); }
    float f32() { const uint32_t b = (uint32_t)le(4); float f; memcpy(&f, &b, 4); return f; }
    double f64() { const uint64_t b = le(8); double d; memcpy(&d, &b, 8); return d; }
    std::string utf()                                          // uint16 length + bytes
    {
        const uint64_t n = le(2);
        if (!need(n)) return std::string();
        std::string s((const char *)image + pos, (size_t)n);
        pos += n;
        return s;
    }
};

inline int gfFileCodecKind(const std::string &id)
{
    // gvrs/GvrsFileSpecification.java:223-229, lsop/LsCodecUtility.java:53, 73
    if (id == "GvrsHuffman") return GF_CODEC_HUFFMAN;
    if (id == "GvrsDeflate") return GF_CODEC_DEFLATE;
    if (id == "GvrsFloat") return GF_CODEC_NONE;
    if (id == "GvrsCanonicalHuffman") return GF_CODEC_CANON_HUFFMAN;
    if (id == "LSOP12") return GF_CODEC_LSOP12;
    if (id == "LSOP08") return GF_CODEC_LSOP08;
    return GF_CODEC_UNKNOWN;
}

// The header record and the directory's prefix of image[0, bytes) -> out.  The statuses: gf_file_open in gvrs_hip_codec.h.
inline gf_status gfFileParse(const uint8_t *image, size_t bytes, GfFileParsed &out)
{
    if (!image) return GF_ERR_ARG;
    out = GfFileParsed();
    gf_file_info &f = out.info;
    memset(&f, 0, sizeof(f));
    if (bytes < 16) return GF_ERR_BOUNDS;
    if (memcmp(image, "gvrs raster\0", 12) != 0) return GF_ERR_FORMAT;
    f.version = image[12], f.subversion = image[13];
    if (f.version != 1 || f.subversion < 2 || f.subversion > 4) return GF_ERR_FORMAT;      // GvrsFileSpecification.isVersionSupported
    if (f.subversion < 4) return GF_ERR_UNSUPPORTED;                                       // (another file head; no fixture exists)
    GfFileCursor head(image, bytes, bytes, 16);
    const int32_t size = head.i32();
    if (head.status != GF_OK) return head.status;
    if (size < 120) return GF_ERR_FORMAT;                                                  // (no room for the fixed fields, the flags and the checksum)
    f.content_pos = 16 + (uint64_t)size;
    if (f.content_pos > bytes) return GF_ERR_BOUNDS;
    // The checksum first, where the specification's flag (a byte at a fixed place) enables it (GvrsFile.java:433-441): a damaged header
    // is GF_ERR_FORMAT whatever its fields then say.  Without the flag the writer leaves the word 0: a header
    // that carries a checksum and says it has none is refused, so that no single damaged byte -- the flag's own included -- opens.
    uint32_t stored;
    memcpy(&stored, image + f.content_pos - 4, 4);                                         // (little-endian hosts, as the library's kernels)
    if (image[GF_FILE_SPEC_POS + 24] != 0 ? gfCrc32c(image + 16, (size_t)size - 4) != stored : stored != 0u) return GF_ERR_FORMAT;
    GfFileCursor c(image, bytes, f.content_pos - 4, 20);
    c.skip(4 + 16 + 8);                                                                    // record type + 3, UUID, time modified
    const uint64_t openedForWriting = c.u64();
    f.freespace_dir_pos = c.u64();
    f.metadata_dir_pos = c.u64();
    const int16_t nLevels = c.i16();
    c.skip(6);
    f.tile_dir_pos = c.u64();
    c.skip(16);
    if (c.status != GF_OK) return c.status;
    if (openedForWriting != 0 || nLevels != 1) return GF_ERR_FORMAT;
    // the specification
    f.grid.n_rows_grid = c.i32(), f.grid.n_cols_grid = c.i32(), f.grid.n_rows_tile = c.i32(), f.grid.n_cols_tile = c.i32();
    c.skip(8);
    f.checksum_enabled = c.u8() != 0, f.raster_space = c.u8(), f.coordinate_system = c.u8();
    c.skip(5);
    f.x0 = c.f64(), f.y0 = c.f64(), f.x1 = c.f64(), f.y1 = c.f64(), f.cell_size_x = c.f64(), f.cell_size_y = c.f64();
    for (double &v : f.m2r) v = c.f64();
    for (double &v : f.r2m) v = c.f64();
    const int32_t nElems = c.i32();
    if (c.status != GF_OK) return c.status;
    if (f.grid.n_rows_grid < 1 || f.grid.n_cols_grid < 1 || f.grid.n_rows_tile < 1 || f.grid.n_cols_tile < 1 || nElems < 1) return GF_ERR_FORMAT;
    if (nElems > GF_MAX_ELEMS) return GF_ERR_UNSUPPORTED;
    f.n_elems = nElems;
    for (int e = 0; e < nElems; e++) {
        gf_elem_spec &el = f.elems[e];
        const int code = c.u8();
        c.skip(1 + 6);                                                                     // continuous, reserved
        out.elemNames.push_back(c.utf());
        c.alignTo4();
        if (c.status != GF_OK) return c.status;
        el.scale = 1.0f;
        switch (code) {
        case 0:                                                                            // INTEGER: min, max, fill
            el.type = GF_ELEM_INT;
            c.skip(8);
            el.fill_i = c.i32();
            break;
        case 1:                                                                            // INT_CODED_FLOAT
            el.type = GF_ELEM_ICF;
            c.skip(8);
            el.fill_f = c.f32(), el.scale = c.f32(), el.offset = c.f32();
            c.skip(8);
            el.fill_i = c.i32();
            break;
        case 2:                                                                            // FLOAT
            el.type = GF_ELEM_FLOAT;
            c.skip(8);
            el.fill_f = c.f32();
            break;
        case 3:                                                                            // SHORT
            el.type = GF_ELEM_SHORT;
            c.skip(4);
            el.fill_i = c.i16();
            break;
        default: return GF_ERR_FORMAT;
        }
        for (int k = 0; k < 3; k++) c.skip(c.le(2));                                       // label, description, unit
        c.alignTo4();
        if (c.status != GF_OK) return c.status;
    }
    const int32_t nCodecs = c.i32();
    if (c.status != GF_OK) return c.status;
    if (nCodecs < 0) return GF_ERR_FORMAT;
    if (nCodecs > 255) return GF_ERR_UNSUPPORTED;
    f.n_codecs = nCodecs;
    for (int k = 0; k < nCodecs; k++) {
        out.codecIds.push_back(c.utf());
        f.codecs[k] = gfFileCodecKind(out.codecIds.back());
    }
    out.productLabel = c.utf();
    if (c.status != GF_OK) return c.status;
    const uint64_t nTilesGrid = (uint64_t)gfTilesOfGrid(f.grid).count();
    if (nTilesGrid > 0x7fffffffull) return GF_ERR_UNSUPPORTED;
    if ((uint64_t)f.grid.n_rows_tile * (uint64_t)f.grid.n_cols_tile >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    // the tile directory's prefix
    const uint64_t P = f.tile_dir_pos;
    if (P == 0 || (P & 7) != 0 || P < f.content_pos + 8 || P > (1ull << 62)) return GF_ERR_FORMAT;
    if (P > bytes || GF_FILE_DIR_PREFIX > bytes - P) return GF_ERR_FORMAT;                 // (a prefix that does not fit the image)
    GfFileCursor d(image, bytes, bytes, P);
    d.skip(1);
    f.dir_extended = d.u8() != 0;
    d.skip(6);
    f.dir_row0 = d.i32(), f.dir_col0 = d.i32(), f.dir_n_rows = d.i32(), f.dir_n_cols = d.i32();
    if (d.status != GF_OK) return d.status;
    f.dir_entries_pos = P + GF_FILE_DIR_PREFIX;
    if (f.dir_row0 < 0 || f.dir_col0 < 0 || f.dir_n_rows < 0 || f.dir_n_cols < 0) return GF_ERR_FORMAT;
    if ((uint64_t)f.dir_n_rows * (uint64_t)f.dir_n_cols > nTilesGrid) return GF_ERR_FORMAT;
    if (f.dir_n_cols == 0 || f.dir_n_rows == 0) f.dir_n_rows = f.dir_n_cols = 0;          // (no entries)
    return GF_OK;
}

// ---- The tile directory of an opened file and the rules of reading through it, for every reader, host and kernel.  A reader
// says how bytes are loaded (GfLoadLe: any host image; GfLoadAligned: an 8-byte aligned image) and keeps its own reaction. ----
struct GfFileDir {
    uint64_t entriesPos, contentPos;        // the first entry (a multiple of 8); where the records begin
    int32_t extended, row0, col0, nRows, nCols;   // entries: int64 positions, else unsigned int32, position = entry * 8; the rectangle of tiles
    int32_t nColsOfTiles;                   // of the grid
};

inline GfFileDir gfFileDirOf(const gf_file_info &f)
{
    GfFileDir d;
    d.entriesPos = f.dir_entries_pos, d.contentPos = f.content_pos;
    d.extended = f.dir_extended, d.row0 = f.dir_row0, d.col0 = f.dir_col0, d.nRows = f.dir_n_rows, d.nCols = f.dir_n_cols;
    d.nColsOfTiles = (int32_t)gfTilesOfGrid(f.grid).cols;
    return d;
}

struct GfLoadLe {
    const uint8_t *image;
    uint64_t word64(uint64_t at) const { return gfLe(image + at, 8); }
    uint32_t word(uint64_t at) const { return (uint32_t)gfLe(image + at, 4); }
    GfU4 head(uint64_t P) const { return GfU4{(uint32_t)gfLe(image + P - 8, 4), (uint32_t)gfLe(image + P - 4, 4), (uint32_t)gfLe(image + P, 4), 0}; }
};
struct GfLoadAligned {                      // at: a multiple of the word's size (little-endian hosts, as the library's kernels)
    const uint8_t *image;
    GF_HD uint64_t word64(uint64_t at) const { return *reinterpret_cast<const uint64_t *>(image + at); }
    GF_HD uint32_t word(uint64_t at) const { return *reinterpret_cast<const uint32_t *>(image + at); }
    // size, type, tile index in ONE 16-byte load at P - 8; it ends at P + 8, inside an image that holds 12 bytes behind a multiple of 8
    GF_HD GfU4 head(uint64_t P) const { return *reinterpret_cast<const GfU4 *>(image + (P - 8)); }
};

// the entry of tile (row, col) of the grid, or of a tile index; -1: the tile lies outside the directory's rectangle
GF_HD int64_t gfDirEntryAt(const GfFileDir &d, int32_t row, int32_t col)
{
    const int32_t tr = row - d.row0, tc = col - d.col0;
    return tr >= 0 && tr < d.nRows && tc >= 0 && tc < d.nCols ? (int64_t)((uint64_t)tr * (uint64_t)d.nCols + (uint64_t)tc) : -1;
}
GF_HD int64_t gfDirEntryOfTile(const GfFileDir &d, int32_t tileIndex) { return gfDirEntryAt(d, tileIndex / d.nColsOfTiles, tileIndex % d.nColsOfTiles); }
// ... and back: the tile index of entry k < nRows * nCols
GF_HD int32_t gfDirTileOfEntry(const GfFileDir &d, uint64_t k)
{
    return (d.row0 + (int32_t)(k / (uint64_t)d.nCols)) * d.nColsOfTiles + d.col0 + (int32_t)(k % (uint64_t)d.nCols);
}
GF_HD bool gfDirEntriesAligned(const GfFileDir &d) { return (d.entriesPos & 7) == 0; }   // what GfLoadAligned needs; gfFileParse's are
// entry k of image[0, bytes): *pos = the content position it holds (0: no such tile); false: the entry lies outside the image
template <class Load>
GF_HD bool gfDirEntryPos(const GfFileDir &d, uint64_t bytes, uint64_t k, uint64_t *pos, Load load)
{
    const uint64_t w = d.extended ? 8u : 4u, at = d.entriesPos + k * w;
    *pos = 0;
    if (at > bytes || w > bytes - at) return false;
    *pos = d.extended ? load.word64(at) : (uint64_t)load.word(at) * 8u;
    return true;
}

// THE PLACE RULE: may the head of the record whose content lies at P be read?  No record lies in the header and a content lies
// behind its 8-byte head; records lie on the 8-byte grid; `behind` bytes from P on lie inside the image: 12 where size, type and
// tile index are read (P - 8 .. P + 4), 0 where only the 8 bytes in front of P are.  The answer: the first clause that fails.
enum GfPlace { GF_PLACE_OK = 0, GF_PLACE_IN_HEADER, GF_PLACE_OFF_GRID, GF_PLACE_BEHIND_END, GF_PLACE_HEAD_CUT };
GF_HD GfPlace gfRecordPlace(uint64_t contentPos, uint64_t bytes, uint64_t P, uint64_t behind)
{
    if (P < contentPos + 8) return GF_PLACE_IN_HEADER;
    if ((P & 7) != 0) return GF_PLACE_OFF_GRID;
    if (P > bytes) return GF_PLACE_BEHIND_END;
    if (behind > bytes - P) return GF_PLACE_HEAD_CUT;
    return GF_PLACE_OK;
}

// One tile looked up through its entry k (gfDirEntryAt / gfDirEntryOfTile): *pos = its entry's position (0: no such tile), *head = the record's size, type and tile-index words when
// GF_OK and present.  An entry outside the image or a position that fails the place rule is GF_ERR_BOUNDS and nothing is read
// there; a head with another tile's index (the entry leads to another tile's record, or to none) is GF_ERR_FORMAT.  The size word
// is NOT judged: a block read leaves it to the framing walk (its host form refuses size < 20, the smallest record with an
// element), an update to gfFsTileRecord (size < 24, the smallest it can free); k_inspect_anchors takes the type's low byte and
// the tile index only, as GvrsInspector reads them.
template <class Load>
GF_HD gf_status gfFileLocateHead(const GfFileDir &d, uint64_t bytes, int64_t k, int32_t tileIndex, uint64_t *pos, GfU4 *head, Load load)
{
    *pos = 0, *head = GfU4{0, 0, 0, 0};
    if (k < 0) return GF_OK;
    if (!gfDirEntryPos(d, bytes, (uint64_t)k, pos, load)) return GF_ERR_BOUNDS;
    if (*pos == 0) return GF_OK;
    if (gfRecordPlace(d.contentPos, bytes, *pos, 12) != GF_PLACE_OK) return GF_ERR_BOUNDS;
    *head = load.head(*pos);
    return (int32_t)head->z == tileIndex ? GF_OK : GF_ERR_FORMAT;
}
// ... in a host image by its index: *size = the size word (0 unless GF_OK and present)
inline gf_status gfFileLocate(const GfFileDir &d, const uint8_t *image, uint64_t bytes, int32_t tileIndex, uint64_t *pos, uint32_t *size)
{
    GfU4 head;
    const gf_status s = gfFileLocateHead(d, bytes, gfDirEntryOfTile(d, tileIndex), tileIndex, pos, &head, GfLoadLe{image});
    *size = s == GF_OK ? head.x : 0;
    return s;
}

// The rectangle of tiles [tileRow0, +nTileRows) x [tileCol0, +nTileCols) looked up in a host image, slot j = row-major:
// each(j, verdict, pos, sizeWord) with gfFileLocate's answers; the caller judges the size word its own way.
template <class Each>
inline void gfFileLocateRect(const GfFileDir &d, const uint8_t *image, uint64_t bytes, int32_t tileRow0, int32_t tileCol0, int32_t nTileRows,
                             int32_t nTileCols, Each each)
{
    for (size_t j = 0; j < (size_t)nTileRows * (size_t)nTileCols; j++) {
        const int32_t tileIndex = (tileRow0 + (int32_t)(j / (size_t)nTileCols)) * d.nColsOfTiles + tileCol0 + (int32_t)(j % (size_t)nTileCols);
        uint64_t pos;
        uint32_t sizeWord;
        const gf_status v = gfFileLocate(d, image, bytes, tileIndex, &pos, &sizeWord);
        each(j, v, pos, sizeWord);
    }
}

#pragma GCC visibility pop
