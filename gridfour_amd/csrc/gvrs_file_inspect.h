// gvrs_file_inspect.h -- a GVRS file image INSPECTED on the host, what GvrsInspector does to a file: every record walked from the
// first byte of content to the end, each judged by its head and, where the specification enables checksums, by its CRC-32C; the
// verdict says whether the file is sound, which tiles are bad and where the walk had to stop.  Host arithmetic on bytes: no HIP
// header, so that tests/csrc/file_inspect_test.cpp runs it under the sanitizers on any machine.  The judgement of ONE record's head
// (gfInspectStepWords) is shared with the kernels of gvrs_file_inspect.hip, which hold to this loop field for field.
// Reference (core/src/main/java/org/gridfour/gvrs/): GvrsInspector.java:213-312 inspectContent, :314-337 testRecordChecksum,
// GvrsFileSpecification.java:546-556 getStandardTileSizeInBytes.  Version 1.04; everything little-endian.
// The checks at one record, in this order (the reference's wherever the reference is defined): a size word of 0 (a clean end), the
// type code, BAD_RECORD_SIZE, the tile index, the tile record's size, TRUNCATED, the checksum.
// DEVIATIONS, where the reference is undefined:
//   a size word < 0, 0 < size < 16 or no multiple of 8 (NegativeArraySizeException, a backward walk or a walk off the 8-byte
//     grid there; RecordManager never writes one): the structural stop GF_INSPECT_BAD_RECORD_SIZE at the record.
//   a record that ends behind the image (EOFException there with checksums; without them the reference walks past the end and
//     reports "complete"): the structural stop GF_INSPECT_TRUNCATED at the record in both modes, not complete.
//   the termination position after a bad type code (stays 16 there): the record's position.
//   testRecordChecksum of a tile directory record with such a size word: false.
// No byte at or behind the image's length is read: every position is judged before it is touched.
#pragma once

#include "gvrs_file_update.h"                                     // (the record type codes)

#pragma GCC visibility push(hidden)

constexpr int GF_INSPECT_NEXT = -1;                               // gfInspectStepWords: the record's head passed, the walk goes on behind it
constexpr uint64_t GF_INSPECT_MIN_SEGMENT = 1024;                 // gf_file_inspect_plan's numbers (the device form's; the host form has no use for them)
constexpr uint64_t GF_INSPECT_MAX_SEGMENTS = 32768;
constexpr uint32_t GF_INSPECT_CRC_CHUNK = 2048;                   // a multiple of 256: 64 lanes, a multiple of 4 bytes each
constexpr uint32_t GF_INSPECT_WAVE_CHUNKS = 8;                    // a record of up to this many chunks is one wave's

struct GfInspectParams {
    uint64_t contentPos, bytes, tileDirPos;
    int64_t maxTileRecordSize;
    int32_t nTiles, checksums;
};

// The head of the record at pos (a position the walk reached: pos <= bytes), judged without its checksum.  GF_INSPECT_END: the walk
// ends in front of it (fewer than 13 bytes left, or a size word of 0) and r is untouched.  Else r = the record as the walk met it
// (checksum -1) and the answer is GF_INSPECT_NEXT or the structural stop.
template <class Load>
GF_HD int gfInspectStepWords(const GfInspectParams &p, uint64_t pos, gf_file_record &r, Load load)
{
    if (p.bytes - pos <= 12) return GF_INSPECT_END;               // (the reference's filePos < fileSize - RECORD_OVERHEAD_SIZE)
    const uint32_t sizeWord = load.word(pos);
    if (sizeWord == 0u) return GF_INSPECT_END;
    const int32_t size = (int32_t)sizeWord, type = (int32_t)(load.word(pos + 4) & 0xffu);
    r.pos = pos, r.size = sizeWord, r.type = type, r.tile_index = -1, r.checksum = -1;
    if (type > 6) return GF_INSPECT_BAD_RECORD_TYPE;
    if (size < 16 || (size & 7) != 0) return GF_INSPECT_BAD_RECORD_SIZE;
    if (type == GF_FILE_REC_TILE) {
        r.tile_index = (int32_t)load.word(pos + 8);
        if (r.tile_index < 0 || r.tile_index >= p.nTiles) return GF_INSPECT_BAD_TILE_INDEX;
        if ((int64_t)size > p.maxTileRecordSize) return GF_INSPECT_TILE_TOO_LARGE;
    }
    if ((uint64_t)size > p.bytes - pos) return GF_INSPECT_TRUNCATED;
    return GF_INSPECT_NEXT;
}

// testRecordChecksum's judgement of the record whose content lies at P, in front of its checksum: true = *size is a size word the
// checksum can be taken over.  P is the header's word: nothing about it is trusted, so the place rule (behind = 0) comes first.
GF_HD bool gfInspectDirHead(const GfInspectParams &p, uint64_t P, uint32_t sizeWord, uint32_t typeWord)
{
    const int32_t size = (int32_t)sizeWord;
    if ((typeWord & 0xffu) > 6u) return false;
    if (size < 16 || (size & 7) != 0) return false;
    return (uint64_t)size <= p.bytes - (P - 8);
}

inline GfInspectParams gfInspectParamsOf(const gf_file_info &f, uint64_t bytes)
{
    GfInspectParams p;
    const uint64_t cells = (uint64_t)f.grid.n_rows_tile * (uint64_t)f.grid.n_cols_tile;
    uint64_t standard = 0;
    for (int e = 0; e < f.n_elems; e++) standard += f.elems[e].type == GF_ELEM_SHORT ? (cells * 2 + 3) & ~3ull : cells * 4;
    p.contentPos = f.content_pos, p.bytes = bytes, p.tileDirPos = f.tile_dir_pos;
    p.maxTileRecordSize = (int64_t)((4 + 4 * (uint64_t)f.n_elems + standard + 12 + 7) & ~7ull);
    p.nTiles = (int32_t)gfTilesOfGrid(f.grid).count();
    p.checksums = f.checksum_enabled != 0;
    return p;
}

// what both forms refuse of an image before they look at a record: not the image that was opened, or content off the 8-byte grid
inline gf_status gfInspectImageCheck(const gf_file_info &f, uint64_t bytes, uint32_t headerSizeWord)
{
    if (bytes < f.content_pos || f.content_pos < 20) return GF_ERR_ARG;
    if (16 + (uint64_t)headerSizeWord != f.content_pos) return GF_ERR_ARG;
    if ((f.content_pos & 7) != 0) return GF_ERR_FORMAT;           // (every record of such a file lies off the grid the kernels read on)
    return GF_OK;
}

// gf_file_inspect_plan's numbers
inline void gfInspectPlan(const gf_file_info &f, uint64_t bytes, uint64_t *segmentBytes, uint64_t *crcChunkBytes, uint64_t *defaultMaxRecords)
{
    const uint64_t span = bytes > f.content_pos ? bytes - f.content_pos : 0;
    const uint64_t seg = std::max<uint64_t>(GF_INSPECT_MIN_SEGMENT, ((span + GF_INSPECT_MAX_SEGMENTS - 1) / GF_INSPECT_MAX_SEGMENTS + 7) & ~7ull);
    if (segmentBytes) *segmentBytes = seg;
    if (crcChunkBytes) *crcChunkBytes = GF_INSPECT_CRC_CHUNK;
    // every tile of the directory once and as many records again (old copies, free nodes, metadata), the three directories, some spare
    if (defaultMaxRecords) *defaultMaxRecords = std::min<uint64_t>(span / 16, 2 * (uint64_t)f.dir_n_rows * (uint64_t)f.dir_n_cols + 64);
}

// gf_file_inspect behind its null checks (gvrs_hip_codec.h has the contract)
inline gf_status gfFileInspect(const gf_file_info &f, const uint8_t *image, uint64_t bytes, gf_file_inspect_report *report, int32_t *badTiles,
                               size_t badCap, gf_file_record *records, size_t recordsCap)
{
    memset(report, 0, sizeof(*report));
    gf_status s = bytes >= 20 ? gfInspectImageCheck(f, bytes, gfLe(image + 16, 4)) : GF_ERR_ARG;
    if (s != GF_OK) return s;
    const GfInspectParams p = gfInspectParamsOf(f, bytes);
    gf_file_inspect_report &o = *report;
    o.tile_dir_located = 1;
    const uint64_t T = p.tileDirPos;
    if (gfRecordPlace(p.contentPos, bytes, T, 0) == GF_PLACE_OK && gfInspectDirHead(p, T, gfLe(image + T - 8, 4), gfLe(image + T - 4, 4))) {
        const uint32_t size = (uint32_t)gfLe(image + T - 8, 4);
        o.tile_dir_passed = gfCrc32c(image + T - 8, size - 4) == gfLe(image + T - 8 + size - 4, 4);
    }
    auto list = [&](const gf_file_record &r) {
        if (records && o.n_records < recordsCap) records[o.n_records] = r;
        o.n_records++;
        if (r.type >= 0 && r.type <= 6) o.n_by_type[r.type]++;
    };
    auto bad = [&](int32_t tile) {
        if (o.n_bad_tiles < badCap) badTiles[o.n_bad_tiles] = tile;
        o.n_bad_tiles++;
    };
    uint64_t pos = p.contentPos;
    bool previousPassed = true;
    o.stop = GF_INSPECT_END;
    for (;;) {
        gf_file_record r;
        const int code = gfInspectStepWords(p, pos, r, GfLoadLe{image});
        if (code == GF_INSPECT_END) {
            o.complete = 1;
            break;
        }
        if (code != GF_INSPECT_NEXT) {
            o.stop = code;
            if (code == GF_INSPECT_TILE_TOO_LARGE) bad(r.tile_index);
            list(r);
            break;
        }
        if (p.checksums) {
            const bool freeNode = r.type == GF_FILE_REC_FREE;
            const uint32_t crc = gfCrc32c(image + pos, freeNode ? 8 : r.size - 4);
            r.checksum = crc == gfLe(image + pos + r.size - 4, 4);
            if (!r.checksum) {
                o.n_checksum_failures++;
                if (r.type == GF_FILE_REC_TILE) bad(r.tile_index);
                if (!previousPassed) {
                    o.stop = GF_INSPECT_TWO_CHECKSUM_FAILURES;
                    list(r);
                    break;
                }
                previousPassed = false;
            } else {
                previousPassed = true;
                if (r.type == GF_FILE_REC_TILE_DIR) o.tile_dir_passed = 1;
            }
        }
        list(r);
        pos += r.size;
    }
    o.termination_pos = pos;
    o.failed = o.stop != GF_INSPECT_END || o.n_checksum_failures != 0;
    o.bad_tile_index = o.stop == GF_INSPECT_BAD_TILE_INDEX;
    o.invalid_record_size = o.stop == GF_INSPECT_TILE_TOO_LARGE;
    o.status = records && o.n_records > recordsCap ? GF_ERR_CAPACITY : GF_OK;
    return (gf_status)o.status;
}

// ---- the powers of x the kernels join checksums with, made by the compiler ----
// crc(A || B) = crc(A) * x^(8 |B|) xor crc(B) (gvrs_crc32c.h).  Square-and-multiply per lane costs some twenty dependent 32-step
// polynomial multiplications a record, which is what a wave per record then spends its time on; so every piece the kernels join
// ends a multiple of 16 bytes in front of its record's last whole 16 bytes, the power comes from a table, and the up to 12 bytes
// behind are run through the byte table at the end.  small[j] = x^(8 * 16 j) for every run of a record one wave takes;
// two[i] = x^(8 * 16 * 2^i) for the chunks of a larger one (a product over the set bits of the distance).
constexpr uint32_t GF_INSPECT_SMALL_POWERS = GF_INSPECT_WAVE_CHUNKS * GF_INSPECT_CRC_CHUNK / 16 + 1;
struct GfInspectPowers {
    uint32_t small[GF_INSPECT_SMALL_POWERS];
    uint32_t two[28];
};
constexpr GfInspectPowers gfInspectMakePowers()
{
    GfInspectPowers t{};
    uint32_t x128 = 0x00800000u;                                  // x^8 ...
    for (int k = 0; k < 4; k++) x128 = gfCrcMulmod(x128, x128);   // ... to the 16th: x^(8 * 16)
    t.small[0] = 0x80000000u;                                     // x^0
    for (uint32_t j = 1; j < GF_INSPECT_SMALL_POWERS; j++) t.small[j] = gfCrcMulmod(t.small[j - 1], x128);
    t.two[0] = x128;
    for (int i = 1; i < 28; i++) t.two[i] = gfCrcMulmod(t.two[i - 1], t.two[i - 1]);
    return t;
}

#if defined(__HIPCC__)
// ---- the device form (gvrs_file_inspect.hip; driven by gvrs_api_file_inspect.hip) ----
constexpr uint64_t GF_INSPECT_NONE = ~0ull;                       // a segment without an anchor; a segment off the chain
constexpr int GF_INSPECT_LINK = -2, GF_INSPECT_OVERSHOOT = -3;    // a segment's walk ended ON a later anchor / behind one
struct GfInspectState {            // zeroed before the kernels; k_inspect_chain's result
    int32_t status, stop;          // GF_K_OK or GF_K_ERR_CAPACITY; the structural stop, GF_INSPECT_END for none
    uint64_t n, term;              // the records up to and including a structural stop; where the walk ended
    uint32_t nLarge, pad_;         // records k_inspect_crc left to k_inspect_crc_large
};
struct GfInspectArgs {
    const uint8_t *image;          // 8-byte aligned
    GfInspectParams p;
    GfFileDir dir;                                   // the tile directory (gvrs_file_parse.h)
    uint64_t metaDirPos, freeDirPos;                 // the header's two other directory positions
    uint64_t segBytes, maxRecords;
    uint32_t nSeg;
    // per segment
    uint64_t *anchor, *landing, *base;               // 0xff before the kernels | where the segment's walk ended | its first record's number
    uint32_t *count;                                 // the records of its walk, a structural stop's record included
    int32_t *stopc;                                  // GF_INSPECT_LINK, _OVERSHOOT, GF_INSPECT_END or the structural stop
    // per record: maxRecords + 1, the last slot the record at the header's tile directory position (tile_dir_passed)
    gf_file_record *recs;
    uint32_t *acc;                                   // zeroed: a large record's checksum, summed chunk by chunk
    uint32_t *large;                                 // the numbers of the large records
    GfInspectState *state;
    gf_file_inspect_report *report;                  // out
    int32_t *badTiles;                               // out: badCap
    uint64_t badCap;
    gf_file_record *records;                         // out, may be null: maxRecords
};
hipError_t gf_launch_file_inspect(const GfInspectArgs &a, hipStream_t stream);
#endif

#pragma GCC visibility pop
