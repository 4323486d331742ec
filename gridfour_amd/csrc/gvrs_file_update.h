// gvrs_file_update.h -- a GVRS file image UPDATED IN PLACE on the host, what GvrsFile(file, "rw") ... close() does to a file that
// exists: the record allocator over the position-ordered free list, the three deallocations of opening, writeTile's placement of
// records in the caller's order and the close sequence with its three directories.  Host arithmetic on bytes: no HIP header, so
// that tests/csrc/file_update_test.cpp runs it under the sanitizers on any machine.  The two serial rules (gfFsDealloc, gfFsAlloc)
// work on plain arrays; the device allocator (k_update_alloc, gvrs_file_update.hip) works the same arrays a wave at a time, shares
// the constants below, and is held to these rules byte for byte by tests/test_gpu_file_update.py.
// Reference (core/src/main/java/org/gridfour/gvrs/): GvrsFile.java:443-483 (opening for writing), :584-616 (close),
// RecordManager.java:218-312 fileSpaceAlloc, :314-384 fileSpaceDealloc, :386-490 writeTile, :864-883 writeTileDirectory, :885-903
// readFreespaceDirectory, :905-989 writeFreeSpaceDirectory, :991-1017 writeMetadataDirectory, :451-454 the sticky extended form,
// TileDirectory.java:121-191 setFilePosition (the rectangle only grows).  Version 1.04; everything little-endian.
//   the free-space directory (record type 3) at content position F: int32 count, then per node int64 position, int32 size
//   a free node (record type 0): [int32 size][0 0 0 0][zeros][CRC-32C of its first 8 bytes | 0]
// A LISTED NODE has at least 24 bytes, not MIN_FREE_BLOCK_SIZE (32): that constant bounds only the surplus of a split, while
// fileSpaceDealloc lists a freed record of any size and merges only make nodes larger.  The smallest record that can be freed is a
// tile record of 24 bytes (a tile index and one element of 4 bytes); every directory record has at least 32.
// The metadata directory is rewritten as it was: no metadata is added or moved, so the reference computes the old content anew and
// the record, allocated at multipleOf8(content + 12), has the old record's size; the old record is kept whole and laid again.
// DEVIATION: with compression enabled, an old record and a new record that is not smaller than the standard form, writeTile has
// freed the old record and zeroed its entry (:429-432) and then writes the standard form into the freed block (:476-480) without
// restoring the entry.  Here every record of a file with compression is freed first and allocated, as for a new tile.
// Not here: adding, changing or removing metadata, versions <= 1.03, the tile cache's flush order, truncating a file whose last
// record became free (the reference does not either).
#pragma once

#include "gvrs_file_emit.h"

#pragma GCC visibility push(hidden)

constexpr uint64_t GF_FS_MIN_SPLIT = 32;                          // RecordManager.MIN_FREE_BLOCK_SIZE
constexpr uint64_t GF_FS_MIN_NODE = 24;                           // the smallest record that can be freed (above)
enum { GF_FILE_REC_FREE = 0, GF_FILE_REC_FREE_DIR = 3 };
constexpr uint64_t GF_FILE_POS_TIME_MODIFIED = 40, GF_FILE_POS_OPENED = 48, GF_FILE_POS_FREE_DIR = 56;

// ---- the serial rules, on a list held as two arrays in order of position: pos[0, n), size[0, n), room for cap nodes ----
GF_HD void gfFsErase(uint64_t *pos, uint64_t *size, uint32_t &n, uint32_t k)
{
    for (uint32_t i = k + 1; i < n; i++) pos[i - 1] = pos[i], size[i - 1] = size[i];
    n--;
}
GF_HD void gfFsInsert(uint64_t *pos, uint64_t *size, uint32_t &n, uint32_t k, uint64_t p, uint64_t s)
{
    for (uint32_t i = n; i > k; i--) pos[i] = pos[i - 1], size[i] = size[i - 1];
    pos[k] = p, size[k] = s;
    n++;
}
// the first node behind position p
GF_HD uint32_t gfFsBehind(const uint64_t *pos, uint32_t n, uint64_t p)
{
    uint32_t k = 0;
    while (k < n && pos[k] <= p) k++;
    return k;
}
// does [p, p + s) overlap a node?  (what a damaged file can ask the allocator to free)
GF_HD bool gfFsOverlaps(const uint64_t *pos, const uint64_t *size, uint32_t n, uint64_t p, uint64_t s)
{
    const uint32_t k = gfFsBehind(pos, n, p);
    return (k > 0 && pos[k - 1] + size[k - 1] > p) || (k < n && p + s > pos[k]);
}
// fileSpaceDealloc of the record [p, p + s): a case is tested only when no earlier one applies.  false: the list is full.
GF_HD bool gfFsDealloc(uint64_t *pos, uint64_t *size, uint32_t &n, uint32_t cap, uint64_t p, uint64_t s)
{
    const uint32_t k = gfFsBehind(pos, n, p);
    if (k > 0 && pos[k - 1] + size[k - 1] == p) {                 // merged with the prior node, and then with the next if they now touch
        size[k - 1] += s;
        if (k < n && pos[k - 1] + size[k - 1] == pos[k]) {
            size[k - 1] += size[k];
            gfFsErase(pos, size, n, k);
        }
        return true;
    }
    if (k < n && p + s == pos[k]) {                               // merged with the next
        pos[k] = p, size[k] += s;
        return true;
    }
    if (n >= cap) return false;
    gfFsInsert(pos, size, n, k, p, s);
    return true;
}
// fileSpaceAlloc of a record of sizeToStore bytes (a multiple of 8): its position; fileSize grows where the file does
GF_HD uint64_t gfFsAlloc(uint64_t *pos, uint64_t *size, uint32_t &n, uint64_t &fileSize, uint64_t sizeToStore)
{
    uint32_t k = 0;
    while (k < n && !(size[k] == sizeToStore || size[k] >= sizeToStore + GF_FS_MIN_SPLIT)) k++;
    if (k == n) {
        if (n > 0 && pos[n - 1] + size[n - 1] == fileSize && size[n - 1] < sizeToStore) {      // the file's last bytes are free: overwritten
            const uint64_t p = pos[n - 1];
            n--;
            fileSize = p + sizeToStore;
            return p;
        }
        const uint64_t p = fileSize;
        fileSize += sizeToStore;
        return p;
    }
    const uint64_t p = pos[k], surplus = size[k] - sizeToStore;
    gfFsErase(pos, size, n, k);
    if (surplus) gfFsInsert(pos, size, n, gfFsBehind(pos, n, p + sizeToStore), p + sizeToStore, surplus);
    return p;
}

// ---- a file opened for an update ----
struct GfFileUpdate {
    gf_file_info info;
    uint64_t imageBytes = 0;
    std::vector<uint64_t> freePos, freeSize;                      // the list after the three deallocations of opening
    std::vector<uint8_t> metaDir;                                 // the old metadata directory record, whole; empty: the file has none
};

// THE RECORD-HEAD RULE: the head of the record whose content lies at P, judged before anything of it is trusted.  The place rule
// with the 8 bytes in front of P -- P is a header's or a directory's word, so one in the header or off the 8-byte grid is damage,
// GF_ERR_FORMAT, and only one behind the image GF_ERR_BOUNDS --, then the type, a size that is a multiple of 8 of at least minSize
// (GF_ERR_FORMAT) and ends inside the image (GF_ERR_BOUNDS).
GF_HD gf_status gfFsHeadWords(uint64_t bytes, uint64_t P, uint32_t sizeWord, uint32_t typeWord, int type, uint64_t minSize, uint64_t *size)
{
    const int32_t s = (int32_t)sizeWord;
    *size = 0;
    if (typeWord != (uint32_t)type || s < (int64_t)minSize || (s & 7) != 0) return GF_ERR_FORMAT;
    if ((uint64_t)s > bytes - (P - 8)) return GF_ERR_BOUNDS;
    *size = (uint64_t)s;
    return GF_OK;
}
template <class Load>
GF_HD gf_status gfFsRecordHead(uint64_t bytes, uint64_t contentPos, uint64_t P, int type, uint64_t minSize, uint64_t *size, Load load)
{
    *size = 0;
    const GfPlace place = gfRecordPlace(contentPos, bytes, P, 0);
    if (place == GF_PLACE_IN_HEADER || place == GF_PLACE_OFF_GRID || P > (1ull << 62)) return GF_ERR_FORMAT;
    if (place != GF_PLACE_OK) return GF_ERR_BOUNDS;
    return gfFsHeadWords(bytes, P, load.word(P - 8), load.word(P - 4), type, minSize, size);
}
// THE TILE-RECORD RULE of an update, host and kernel: a tile's old record found through the directory (gfFileLocateHead, whose
// place rule covers the head's) and the head it loaded judged before the record is freed or rewritten.  *pos = 0: no such tile.
template <class Load>
GF_HD gf_status gfFsTileRecord(const GfFileDir &d, uint64_t bytes, int32_t tileIndex, uint64_t *pos, uint64_t *size, Load load)
{
    GfU4 head;
    const gf_status v = gfFileLocateHead(d, bytes, gfDirEntryOfTile(d, tileIndex), tileIndex, pos, &head, load);
    *size = 0;
    return v == GF_OK && *pos != 0 ? gfFsHeadWords(bytes, *pos, head.x, head.y, GF_FILE_REC_TILE, 24, size) : v;
}

// gf_file_update_begin behind its null checks: info = the gf_file_info gf_file_open made of this image
inline gf_status gfFileUpdateBegin(const gf_file_info &info, const uint8_t *image, uint64_t bytes, GfFileUpdate &u)
{
    u = GfFileUpdate();
    u.info = info;
    u.imageBytes = bytes;
    if (bytes < info.content_pos || info.content_pos < 20) return GF_ERR_ARG;
    if (16 + gfLe(image + 16, 4) != info.content_pos) return GF_ERR_ARG;                   // (not the image that was opened)
    if ((bytes & 7) != 0 || (info.content_pos & 7) != 0) return GF_ERR_FORMAT;               // (records are appended at the image's end)
    gf_status s;
    uint64_t size;
    uint32_t n = 0;
    // the free-space directory read into the list
    const uint64_t F = info.freespace_dir_pos, M = info.metadata_dir_pos, T = info.tile_dir_pos;
    uint64_t freeDirSize = 0;
    if (F != 0) {
        if ((s = gfFsRecordHead(bytes, info.content_pos, F, GF_FILE_REC_FREE_DIR, 16, &freeDirSize, GfLoadLe{image})) != GF_OK) return s;
        const int32_t count = (int32_t)(uint32_t)gfLe(image + F, 4);                       // (16 bytes of record: the word is inside)
        if (count < 0 || 4 + 12 * (uint64_t)count > freeDirSize - 12) return GF_ERR_FORMAT;  // (a count the record can hold)
        u.freePos.resize((size_t)count + 3), u.freeSize.resize((size_t)count + 3);
        uint64_t end = info.content_pos;
        for (int32_t k = 0; k < count; k++) {
            const uint64_t p = gfLe(image + F + 4 + 12 * (uint64_t)k, 8);
            const int32_t z = (int32_t)(uint32_t)gfLe(image + F + 12 + 12 * (uint64_t)k, 4);
            if ((p & 7) != 0 || (z & 7) != 0 || z < (int64_t)GF_FS_MIN_NODE) return GF_ERR_FORMAT;
            if (p < end || (k > 0 && p == end)) return GF_ERR_FORMAT;                        // ascending; no two nodes overlap or touch
            if (p > bytes || (uint64_t)z > bytes - p) return GF_ERR_BOUNDS;
            if (gfLe(image + p, 4) != (uint64_t)z || gfLe(image + p + 4, 4) != GF_FILE_REC_FREE) return GF_ERR_FORMAT;
            u.freePos[(size_t)k] = p, u.freeSize[(size_t)k] = (uint64_t)z;
            end = p + (uint64_t)z;
        }
        n = (uint32_t)count;
    } else {
        u.freePos.resize(3), u.freeSize.resize(3);
    }
    const uint32_t cap = (uint32_t)u.freePos.size();
    // the three directory records freed, in the reference's order
    if (F != 0) {
        if (gfFsOverlaps(u.freePos.data(), u.freeSize.data(), n, F - 8, freeDirSize)) return GF_ERR_FORMAT;
        gfFsDealloc(u.freePos.data(), u.freeSize.data(), n, cap, F - 8, freeDirSize);
    }
    if (M != 0) {
        if ((s = gfFsRecordHead(bytes, info.content_pos, M, GF_FILE_REC_METADATA_DIR, 16, &size, GfLoadLe{image})) != GF_OK) return s;
        if (gfFsOverlaps(u.freePos.data(), u.freeSize.data(), n, M - 8, size)) return GF_ERR_FORMAT;
        u.metaDir.assign(image + M - 8, image + M - 8 + size);
        gfFsDealloc(u.freePos.data(), u.freeSize.data(), n, cap, M - 8, size);
    }
    if ((s = gfFsRecordHead(bytes, info.content_pos, T, GF_FILE_REC_TILE_DIR, 40, &size, GfLoadLe{image})) != GF_OK) return s;
    const uint64_t nEntries = (uint64_t)info.dir_n_rows * (uint64_t)info.dir_n_cols;
    const GfTilesOfGrid tiles = gfTilesOfGrid(info.grid);
    if (nEntries != 0 && ((int64_t)info.dir_row0 + info.dir_n_rows > tiles.rows || (int64_t)info.dir_col0 + info.dir_n_cols > tiles.cols))
        return GF_ERR_FORMAT;                                                                // (a rectangle of tiles the grid does not have)
    if (gfFileTileDirSize(nEntries, info.dir_extended != 0) > size) return GF_ERR_FORMAT;    // (the entries lie inside the record)
    if (gfFsOverlaps(u.freePos.data(), u.freeSize.data(), n, T - 8, size)) return GF_ERR_FORMAT;
    gfFsDealloc(u.freePos.data(), u.freeSize.data(), n, cap, T - 8, size);
    u.freePos.resize(n), u.freeSize.resize(n);
    return GF_OK;
}

// gf_file_update_plan's two numbers: nTiles = the tiles written, maxRecordBytes = gf_tile_record_max_bytes_elems of a tile
inline void gfFileUpdatePlan(const GfFileUpdate &u, uint64_t nTiles, uint64_t maxRecordBytes, uint64_t *maxImageBytes, uint64_t *listCapacity)
{
    const uint64_t tilesOfGrid = (uint64_t)gfTilesOfGrid(u.info.grid).count();
    const uint64_t cap = u.freePos.size() + nTiles + 3;
    if (listCapacity) *listCapacity = cap;
    if (maxImageBytes)
        *maxImageBytes = u.imageBytes + nTiles * maxRecordBytes + u.metaDir.size() + gfFileTileDirSize(tilesOfGrid, true) + gfFileRecordSize(4 + 12 * cap);
}

// gf_file_update_assemble behind its null checks (gvrs_hip_codec.h has the contract).  Everything is decided before the first
// byte is written: a refusal or an image that does not fit leaves the image as it was.
inline gf_status gfFileUpdateAssemble(const GfFileUpdate &u, uint8_t *image, uint64_t imageCap, const uint8_t *blob, const uint64_t *offsets,
                                      const int32_t *tileIndices, const int32_t *status, size_t nRecords, int64_t timeModified, int flags,
                                      uint64_t *imageBytes)
{
    *imageBytes = 0;
    if (imageCap < u.imageBytes) return GF_ERR_ARG;
    const gf_file_info &f = u.info;
    const GfFileDir d = gfFileDirOf(f);
    const int64_t nColsOfTiles = d.nColsOfTiles;
    const int64_t nTiles = gfTilesOfGrid(f.grid).count();
    const bool compression = f.n_codecs > 0, checksums = f.checksum_enabled != 0;
    // the records: what gf_file_assemble refuses, and two records for one tile
    std::vector<int32_t> seen(tileIndices, tileIndices + nRecords);
    for (size_t r = 0; r < nRecords; r++) {
        if (offsets[r + 1] < offsets[r] || tileIndices[r] < 0 || tileIndices[r] >= nTiles) return GF_ERR_ARG;
        const uint64_t len = offsets[r + 1] - offsets[r];
        if (len != 0 && ((len & 7) != 0 || len < 24 || len > 0x7fffffffull || !blob)) return GF_ERR_ARG;
    }
    std::sort(seen.begin(), seen.end());
    for (size_t k = 1; k < seen.size(); k++)
        if (seen[k] == seen[k - 1]) return GF_ERR_ARG;
    // writeTile's placement, record by record in the caller's order, on a copy of the list
    struct Placed { int32_t tile; uint64_t pos; size_t record; };                       // pos: the content position, 0 for a freed tile
    std::vector<Placed> placed;
    std::vector<uint64_t> pos(u.freePos), size(u.freeSize);
    uint32_t n = (uint32_t)pos.size();
    const uint32_t cap = (uint32_t)(n + nRecords + 3);
    pos.resize(cap), size.resize(cap);
    uint64_t fileSize = u.imageBytes;
    bool extended = f.dir_extended != 0 || (flags & GF_FILE_DIR_EXTENDED) != 0;
    const bool oldEmpty = d.nRows == 0 || d.nCols == 0;
    int64_t r0 = oldEmpty ? INT_MAX : d.row0, r1 = oldEmpty ? -1 : d.row0 + d.nRows - 1;
    int64_t c0 = oldEmpty ? INT_MAX : d.col0, c1 = oldEmpty ? -1 : d.col0 + d.nCols - 1;
    for (size_t r = 0; r < nRecords; r++) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        const int32_t st = status ? status[r] : len ? GF_OK : GF_DECLINED;
        if (st < 0) continue;                                                            // the tile stays as it is: record and entry
        uint64_t oldPos, oldSize;
        const gf_status v = gfFsTileRecord(d, u.imageBytes, tileIndices[r], &oldPos, &oldSize, GfLoadLe{image});
        if (v != GF_OK) return v;
        const bool inPlace = len != 0 && !compression && oldPos != 0;
        if (inPlace) {
            if (len != oldSize) return GF_ERR_ARG;                                       // (a standard record has one size)
            placed.push_back(Placed{tileIndices[r], oldPos, r});
            continue;
        }
        if (oldPos != 0) {
            if (gfFsOverlaps(pos.data(), size.data(), n, oldPos - 8, oldSize)) return GF_ERR_FORMAT;
            gfFsDealloc(pos.data(), size.data(), n, cap, oldPos - 8, oldSize);
        }
        if (len == 0) {
            if (oldPos != 0) placed.push_back(Placed{tileIndices[r], 0, r});
            continue;
        }
        const uint64_t p = gfFsAlloc(pos.data(), size.data(), n, fileSize, len) + 8;
        extended |= p > GF_FILE_MAX_COMPACT_POS;
        const int64_t tr = tileIndices[r] / nColsOfTiles, tc = tileIndices[r] % nColsOfTiles;
        r0 = std::min(r0, tr), r1 = std::max(r1, tr), c0 = std::min(c0, tc), c1 = std::max(c1, tc);
        placed.push_back(Placed{tileIndices[r], p, r});
    }
    // close: the metadata directory, the tile directory, the free-space directory with its second count
    const uint64_t metaDirAt = u.metaDir.empty() ? 0 : gfFsAlloc(pos.data(), size.data(), n, fileSize, u.metaDir.size());
    const bool empty = r1 < 0;
    const int32_t nRows = empty ? 0 : (int32_t)(r1 - r0 + 1), nCols = empty ? 0 : (int32_t)(c1 - c0 + 1);
    if (empty) r0 = d.row0, c0 = d.col0;
    const uint64_t nEntries = (uint64_t)nRows * (uint64_t)nCols, tileDirSize = gfFileTileDirSize(nEntries, extended);
    if (tileDirSize > 0x7fffffffull) return GF_ERR_UNSUPPORTED;                          // (a record's size is an int32)
    const uint64_t tileDirAt = gfFsAlloc(pos.data(), size.data(), n, fileSize, tileDirSize);
    uint64_t freeDirAt = 0, freeDirSize = 0;
    const bool hasFreeDir = n != 0;
    if (hasFreeDir) {
        freeDirSize = gfFileRecordSize(4 + 12 * (uint64_t)n);
        if (freeDirSize > 0x7fffffffull) return GF_ERR_UNSUPPORTED;
        freeDirAt = gfFsAlloc(pos.data(), size.data(), n, fileSize, freeDirSize);
    }
    for (uint32_t k = 0; k < n; k++)
        if (size[k] > 0x7fffffffull) return GF_ERR_UNSUPPORTED;                          // (a node's size is an int32 in its record and its directory)
    *imageBytes = fileSize;
    if (fileSize > imageCap) return GF_ERR_CAPACITY;
    // ---- from here on the image is written ----
    // the old entries first: the old directory record is free space since opening and may lie under a new record
    std::vector<uint64_t> positions((size_t)nEntries, 0);
    // (they lie inside the old image: gfFileUpdateBegin has checked the old directory record against its rectangle)
    for (uint64_t k = 0; k < (uint64_t)d.nRows * (uint64_t)d.nCols; k++) {
        const int64_t t = gfDirTileOfEntry(d, k);
        gfDirEntryPos(d, u.imageBytes, k, &positions[(size_t)((t / nColsOfTiles - r0) * nCols + (t % nColsOfTiles - c0))], GfLoadLe{image});
    }
    for (const Placed &p : placed) {
        positions[(size_t)((p.tile / nColsOfTiles - r0) * nCols + (p.tile % nColsOfTiles - c0))] = p.pos;
        if (p.pos != 0) memcpy(image + p.pos - 8, blob + offsets[p.record], (size_t)(offsets[p.record + 1] - offsets[p.record]));
    }
    if (!u.metaDir.empty()) memcpy(image + metaDirAt, u.metaDir.data(), u.metaDir.size());
    std::vector<uint8_t> rec;
    gfFileEmitTileDir(extended, (int32_t)r0, (int32_t)c0, nRows, nCols, positions.data(), checksums, rec);
    memcpy(image + tileDirAt, rec.data(), rec.size());
    if (hasFreeDir) {
        rec.clear();
        GfFileOut o(rec);
        o.zeros(8);
        o.i32((int32_t)n);
        for (uint32_t k = 0; k < n; k++) o.i64(pos[k]), o.i32((int32_t)size[k]);
        gfFileCloseRecord(rec, 0, GF_FILE_REC_FREE_DIR, checksums, false, (size_t)freeDirSize);
        memcpy(image + freeDirAt, rec.data(), rec.size());
    }
    for (uint32_t k = 0; k < n; k++) {                                                   // every free node: head, zeros, checksum of the head
        uint8_t *p = image + pos[k];
        memset(p, 0, (size_t)size[k]);
        gfPutLe(p, size[k], 4);
        if (checksums) gfPutLe(p + size[k] - 4, gfCrc32c(p, 8), 4);
    }
    gfPutLe(image + GF_FILE_POS_TIME_MODIFIED, (uint64_t)timeModified, 8);
    gfPutLe(image + GF_FILE_POS_OPENED, 0, 8);
    gfPutLe(image + GF_FILE_POS_FREE_DIR, hasFreeDir ? freeDirAt + 8 : 0, 8);
    gfPutLe(image + GF_FILE_POS_METADATA_DIR, u.metaDir.empty() ? 0 : metaDirAt + 8, 8);
    gfPutLe(image + GF_FILE_POS_TILE_DIR, tileDirAt + 8, 8);
    if (checksums) gfPutLe(image + f.content_pos - 4, gfCrc32c(image + 16, (size_t)f.content_pos - 16 - 4), 4);
    return GF_OK;
}

#pragma GCC visibility pop
