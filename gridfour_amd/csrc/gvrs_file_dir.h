// gvrs_file_dir.h -- what the kernels of a write (gvrs_file_write.hip) and of an update (gvrs_file_update.hip) lay into an image in
// the same way: the tile directory's record -- its words, its CRC-32C in chunks of GF_FILE_CRC_CHUNK bytes and their fold -- and the
// fields of the header record a finish kernel computes, with the header's checksum over them.  gvrs_file_emit.h is the host's twin
// (gfFileEmitTileDir, gfFileCrc32cChunked, gfFileFinishHeader).  Device code; plain vector stores only.
// Reference: gvrs/RecordManager.java:864-883 (writeTileDirectory), gvrs/TileDirectory.java:266-290, gvrs/TileDirectoryExtended.java
// (writeTilePositions), gvrs/GvrsFile.java:584-616 (close: positions, header checksum).
#pragma once

#include "gvrs_crc32c.h"
#include "gvrs_file_emit.h"

struct GfTileDirRec {
    uint64_t at, size;                 // the record's position (a multiple of 8; its content lies 8 behind) and its size
    uint32_t extended, row0, col0, nRows, nCols;
};

// Word w < d.size / 8 of the record, one 8-byte store: word 0 the size and type words, word 1 the prefix with the extended flag, words
// 2 and 3 the rectangle, then the entries -- two compact ones or one extended one a word -- and the zero padding.  entry(row, col) =
// the content position of that tile's record, 0 for none.  The record's last 4 bytes are its checksum: with checksums the last
// word's first 4 bytes are stored alone and tile_dir_fold stores the checksum, so every byte is written once.
template <class Entry>
__device__ __forceinline__ void tile_dir_store_word(uint8_t *image, const GfTileDirRec &d, uint64_t w, bool checksums, Entry entry)
{
    const auto pos = [&](uint64_t k) -> uint64_t {
        if (k >= (uint64_t)d.nRows * d.nCols) return 0;
        const uint32_t dr = (uint32_t)(k / d.nCols), dc = (uint32_t)(k - (uint64_t)dr * d.nCols);
        return entry(d.row0 + dr, d.col0 + dc);
    };
    uint32_t lo, hi;
    if (w == 0u) lo = (uint32_t)d.size, hi = (uint32_t)GF_FILE_REC_TILE_DIR;
    else if (w == 1u) lo = d.extended << 8, hi = 0u;
    else if (w == 2u) lo = d.row0, hi = d.col0;
    else if (w == 3u) lo = d.nRows, hi = d.nCols;
    else if (d.extended) {
        const uint64_t p = pos(w - 4u);
        lo = (uint32_t)p, hi = (uint32_t)(p >> 32);
    } else {
        lo = (uint32_t)(pos(2u * (w - 4u)) >> 3);
        hi = (uint32_t)(pos(2u * (w - 4u) + 1u) >> 3);
    }
    uint8_t *dst = image + d.at + 8u * w;
    if (w == d.size / 8u - 1u && checksums) *reinterpret_cast<uint32_t *>(dst) = lo;
    else *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
}

// One wave's chunk: chunkCrc[c] = the CRC-32C of chunk c of the record without its last word (the bytes tile_dir_store_word wrote:
// every chunk a multiple of 4 long), where the record has such a chunk
__device__ __forceinline__ void tile_dir_chunk_crc(const uint32_t *table, const uint8_t *image, const GfTileDirRec &d, uint64_t c, uint32_t lane,
                                                   uint32_t *chunkCrc)
{
    const uint64_t nBytes = d.size - 4u;
    if (c * GF_FILE_CRC_CHUNK >= nBytes) return;
    const uint64_t left = nBytes - c * GF_FILE_CRC_CHUNK;
    const uint32_t n4 = (uint32_t)(left < GF_FILE_CRC_CHUNK ? left : GF_FILE_CRC_CHUNK) / 4u;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(image + d.at + c * GF_FILE_CRC_CHUNK);
    const uint32_t crc = wave_crc_words(table, n4, lane, [&](uint32_t i) { return src[i]; });
    if (lane == 0u) chunkCrc[c] = crc;
}

// The chunks' checksums folded in order by one wave -- chunk c weighs x^(8 * bytes behind it), the sum of crc(A || B) =
// crc(A) * x^(8 |B|) xor crc(B) over all chunks -- into the record's last word
__device__ __forceinline__ void tile_dir_fold(uint8_t *image, const GfTileDirRec &d, const uint32_t *chunkCrc, uint32_t lane)
{
    const uint64_t nBytes = d.size - 4u, nChunks = (nBytes + GF_FILE_CRC_CHUNK - 1u) / GF_FILE_CRC_CHUNK;
    uint32_t part = 0;
    for (uint64_t c = lane; c < nChunks; c += 64u) {
        const uint64_t end = min(nBytes, (c + 1u) * GF_FILE_CRC_CHUNK);
        part ^= gfCrcMulmod(gfCrcXpow8n((uint32_t)(nBytes - end)), chunkCrc[c]);
    }
    part = wave_xor(part);
    if (lane == 0u) *reinterpret_cast<uint32_t *>(image + d.at + nBytes) = part;
}

// ---- the 8-byte fields of the header record a finish kernel computes: ONE list a kernel, for the checksum and for the stores ----
struct GfHeadField {
    uint32_t at;                       // the field's file position (GF_FILE_POS_*)
    uint64_t value;
};
template <int N>
__device__ __forceinline__ bool head_computed(const GfHeadField (&f)[N], uint32_t at)    // does the word at file position `at` belong to one?
{
    bool is = false;
#pragma unroll
    for (int k = 0; k < N; k++) is |= at - f[k].at < 8u;
    return is;
}
// the CRC-32C of the n4 words at file position 16 with the fields in place: word(i) = word i as it lies (no store is read back)
template <int N, class Word>
__device__ __forceinline__ uint32_t head_crc(const uint32_t *table, uint32_t n4, uint32_t lane, const GfHeadField (&f)[N], Word word)
{
    return wave_crc_words(table, n4, lane, [&](uint32_t i) -> uint32_t {
        const uint32_t at = 16u + 4u * i;
        bool is = false;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const uint32_t in = at - f[k].at;                     // 0 or 4 inside the field
            if (in < 8u) is = true, v = (uint32_t)(f[k].value >> (8u * in));
        }
        return is ? v : word(i);
    });
}
template <int N>
__device__ __forceinline__ void head_store(uint8_t *image, const GfHeadField (&f)[N])    // by one lane
{
#pragma unroll
    for (int k = 0; k < N; k++) *reinterpret_cast<uint64_t *>(image + f[k].at) = f[k].value;
}
