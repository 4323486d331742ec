// gvrs_file_write.hip -- a GVRS file image finished in device memory, behind the record writer (gvrs_records_enc.hip) that has laid
// the tile records into it: the bounding rectangle of the tiles with a record and the extended decision (k_file_dir_rect), the tile
// directory's record (k_file_dir_entries), its CRC-32C in chunks (k_file_dir_crc), and the rest (k_file_finish): the metadata
// directory copied to its place, the chunks' checksums folded, the two directory positions patched into the header record, its
// checksum, the image's size and status, and last the 16 bytes of the file head; a short front (header and metadata records,
// metadata directory) arrives in its arguments and is written by it too.  gvrs_file_emit.h is the host's twin of every
// byte written here and holds GF_FILE_CRC_CHUNK.  Plain vector stores only.
// Reference: gvrs/RecordManager.java:864-883 (writeTileDirectory), :87, 451-454 (the extended decision), gvrs/TileDirectory.java:
// 266-290, gvrs/TileDirectoryExtended.java (writeTilePositions), gvrs/GvrsFile.java:584-616 (close: positions, header checksum).

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_crc32c.h"
#include "gvrs_file_emit.h"

namespace {

// What every kernel behind k_file_dir_rect derives from the state it left: the directory's rectangle and form, and where things lie.
struct FileLayout {
    uint32_t row0, col0, nRows, nCols;
    uint64_t nEntries;
    uint32_t extended;
    uint64_t dirSize;                  // the tile directory's record
    uint64_t recordsEnd, tileDirStart, total;
    bool fits;                         // total <= imageCap: the records were all written and both directories have room
};

__device__ __forceinline__ FileLayout file_layout(const GfFileWriteArgs &a)
{
    const GfFileWriteState s = *a.state;
    FileLayout l;
    const bool any = s.row1p != 0u;
    l.row0 = any ? ~s.invRow0 : 0u, l.col0 = any ? ~s.invCol0 : 0u;
    l.nRows = any ? s.row1p - l.row0 : 0u, l.nCols = any ? s.col1p - l.col0 : 0u;
    l.nEntries = (uint64_t)l.nRows * (uint64_t)l.nCols;
    l.extended = (a.forceExtended || s.extended) ? 1u : 0u;
    l.dirSize = (8u + 16u + l.nEntries * (l.extended ? 8u : 4u) + 12u + 7u) & ~7ull;
    l.recordsEnd = a.firstRecordPos + a.offsets[(uint64_t)a.nTileRows * (uint64_t)a.nTileCols];
    l.tileDirStart = l.recordsEnd + a.metaDirBytes;
    l.total = l.tileDirStart + l.dirSize;
    l.fits = l.total <= a.imageCap;
    return l;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, gf_lane_xor(v, o));
    return v;
}

// ------------------------------------------------------------------------------------------------
// k_file_dir_rect: a lane per slot.  A slot has a record when its length is not 0 (a tile that failed or was declined has none).
// The wave reduces ~row, ~col, row + 1, col + 1 of its slots with a record by max (0 for the others: ~row of a tile row is never
// 0) and lane 0 sends each to the state with one atomic; the extended decision -- a content position above 1 << 35 -- by or.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_dir_rect(const GfFileWriteArgs a)
{
    const uint64_t n = (uint64_t)a.nTileRows * (uint64_t)a.nTileCols, j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t invRow = 0, invCol = 0, row1p = 0, col1p = 0, ext = 0;
    if (j < n) {
        const uint64_t o0 = a.offsets[j], o1 = a.offsets[j + 1];
        if (o1 != o0) {
            const uint32_t ty = (uint32_t)(j / (uint32_t)a.nTileCols), tx = (uint32_t)(j - (uint64_t)ty * (uint32_t)a.nTileCols);
            const uint32_t row = (uint32_t)a.tileRow0 + ty, col = (uint32_t)a.tileCol0 + tx;
            invRow = ~row, invCol = ~col, row1p = row + 1u, col1p = col + 1u;
            ext = a.firstRecordPos + o0 + 8u > GF_FILE_MAX_COMPACT_POS ? 1u : 0u;
        }
    }
    invRow = wave_max(invRow), invCol = wave_max(invCol), row1p = wave_max(row1p), col1p = wave_max(col1p), ext = wave_max(ext);
    if ((threadIdx.x & 63u) == 0u && row1p != 0u) {
        atomicMax(&a.state->invRow0, invRow);
        atomicMax(&a.state->invCol0, invCol);
        atomicMax(&a.state->row1p, row1p);
        atomicMax(&a.state->col1p, col1p);
        if (ext) atomicOr(&a.state->extended, 1u);
    }
}

// the content position of entry k of the directory: its tile's slot in the rectangle of tiles, 0 for a slot without a record
__device__ __forceinline__ uint64_t entry_pos(const GfFileWriteArgs &a, const FileLayout &l, uint64_t k)
{
    if (k >= l.nEntries) return 0;
    const uint32_t dr = (uint32_t)(k / l.nCols), dc = (uint32_t)(k - (uint64_t)dr * l.nCols);
    const uint64_t j = (uint64_t)(l.row0 + dr - (uint32_t)a.tileRow0) * (uint32_t)a.nTileCols + (l.col0 + dc - (uint32_t)a.tileCol0);
    const uint64_t o0 = a.offsets[j], o1 = a.offsets[j + 1];
    return o1 != o0 ? a.firstRecordPos + o0 + 8u : 0u;
}

// ------------------------------------------------------------------------------------------------
// k_file_dir_entries: a lane per 8-byte word of the directory's record, one 8-byte store each (the record starts at a multiple
// of 8): word 0 the size and type words, word 1 the prefix with the extended flag, words 2 and 3 the rectangle, then the entries --
// two compact ones or one extended one a word -- and the zero padding.  The record's last 4 bytes are its checksum: with checksums
// the lane of the last word stores its first 4 bytes alone and k_file_finish stores the checksum, so every byte is written once.
// Nothing is written when the image does not fit.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_dir_entries(const GfFileWriteArgs a)
{
    const FileLayout l = file_layout(a);
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x, nWords = l.dirSize / 8u;
    if (!l.fits || w >= nWords) return;
    uint32_t lo, hi;
    if (w == 0u) lo = (uint32_t)l.dirSize, hi = (uint32_t)GF_FILE_REC_TILE_DIR;
    else if (w == 1u) lo = l.extended << 8, hi = 0u;
    else if (w == 2u) lo = l.row0, hi = l.col0;
    else if (w == 3u) lo = l.nRows, hi = l.nCols;
    else if (l.extended) {
        const uint64_t p = entry_pos(a, l, w - 4u);
        lo = (uint32_t)p, hi = (uint32_t)(p >> 32);
    } else {
        lo = (uint32_t)(entry_pos(a, l, 2u * (w - 4u)) >> 3);
        hi = (uint32_t)(entry_pos(a, l, 2u * (w - 4u) + 1u) >> 3);
    }
    uint8_t *dst = a.image + l.tileDirStart + 8u * w;
    if (w == nWords - 1u && a.checksums) *reinterpret_cast<uint32_t *>(dst) = lo;
    else *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
}

__device__ __forceinline__ uint32_t crc_word(const uint32_t *table, uint32_t crc, uint32_t w)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        crc = table[(crc ^ w) & 0xffu] ^ (crc >> 8);
        w >>= 8;
    }
    return crc;
}

// the CRC-32C of n4 words that word(i) delivers, by the whole wave: lane l takes the l-th of 64 runs, the runs are joined as
// gvrs_crc32c.h says.  Every lane returns the checksum.
template <class Word>
__device__ __forceinline__ uint32_t wave_crc_words(const uint32_t *table, uint32_t n4, uint32_t lane, Word word)
{
    const uint32_t per = (n4 + 63u) / 64u, begin = min(n4, lane * per), end = min(n4, begin + per);
    uint32_t crc = 0xffffffffu;
    for (uint32_t i = begin; i < end; i++) crc = crc_word(table, crc, word(i));
    crc ^= 0xffffffffu;                                                       // the run's own checksum (an empty run: 0)
    uint32_t part = crc_mulmod(crc_xpow8n(4u * (n4 - end)), crc);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part ^= gf_lane_xor(part, o);
    return part;
}

// ------------------------------------------------------------------------------------------------
// k_file_dir_crc: a wave per chunk of GF_FILE_CRC_CHUNK bytes of the directory's record without its last word (the bytes
// k_file_dir_entries wrote: every one a multiple of 4 long), four waves a workgroup around the byte table in LDS.  chunkCrc[c] = the
// chunk's own CRC-32C; k_file_finish folds them.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_dir_crc(const GfFileWriteArgs a)
{
    __shared__ uint32_t table[256];
    table[threadIdx.x] = crc_table_entry(threadIdx.x);
    __syncthreads();
    const FileLayout l = file_layout(a);
    const uint64_t nBytes = l.dirSize - 4u, c = (uint64_t)blockIdx.x * 4u + gf_wave_id();
    if (!l.fits || c * GF_FILE_CRC_CHUNK >= nBytes) return;
    const uint64_t left = nBytes - c * GF_FILE_CRC_CHUNK;
    const uint32_t n4 = (uint32_t)(left < GF_FILE_CRC_CHUNK ? left : GF_FILE_CRC_CHUNK) / 4u, lane = threadIdx.x & 63u;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.image + l.tileDirStart + c * GF_FILE_CRC_CHUNK);
    const uint32_t crc = wave_crc_words(table, n4, lane, [&](uint32_t i) { return src[i]; });
    if (lane == 0u) a.chunkCrc[c] = crc;
}

// ------------------------------------------------------------------------------------------------
// k_file_finish: ONE wave.  The image's size and status first.  An image that does not fit gets nothing more than zeros in the
// bytes of the file head that lie in front of imageCap: it does not open.  Else the metadata directory's record goes to its place
// behind the records (8-byte words), the chunks' checksums are folded in order -- chunk c weighs x^(8 * bytes behind it), the sum
// of crc(A || B) = crc(A) * x^(8 |B|) xor crc(B) over all chunks -- into the directory's last word, the two positions go into the
// header record and its checksum is computed over the record with them in place (the words are substituted as they are read: no
// store of this kernel is read back), and last the file head.
// IN_ARGS: the front -- the image's bytes [16, firstRecordPos) and the metadata directory -- lies in the kernel's arguments
// (front(i) = its word i) and is written here too, every word but the five this kernel computes; else it was copied to the image
// and to a.metaDir before the kernels ran.
// ------------------------------------------------------------------------------------------------
template <bool IN_ARGS, class Front>
__device__ __forceinline__ void file_finish(const GfFileWriteArgs &a, uint32_t *table, Front front)
{
    const uint32_t lane = threadIdx.x;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) table[lane + 64u * i] = crc_table_entry(lane + 64u * i);
    __syncthreads();
    const FileLayout l = file_layout(a);
    if (lane == 0u) {
        *a.imageBytes = l.total;
        *a.fileStatus = l.fits ? GF_K_OK : GF_K_ERR_CAPACITY;
    }
    if (!l.fits) {
        if (lane < 16u && lane < a.imageCap) a.image[lane] = 0;
        return;
    }
    const uint32_t frontWords = (uint32_t)(a.firstRecordPos - 16u) / 4u, crcWord = (uint32_t)(a.contentPos - 16u - 4u) / 4u;
    // the header record and the metadata records (the positions and the checksum: below)
    if (IN_ARGS) {
        uint32_t *to = reinterpret_cast<uint32_t *>(a.image + 16u);
        for (uint32_t i = lane; i < frontWords; i += 64u) {
            const uint32_t at = 16u + 4u * i;
            const bool computed = (at - (uint32_t)GF_FILE_POS_METADATA_DIR < 8u) || (at - (uint32_t)GF_FILE_POS_TILE_DIR < 8u) || i == crcWord;
            if (!computed) to[i] = front(i);
        }
    }
    // the metadata directory
    if (IN_ARGS) {
        uint32_t *mdTo = reinterpret_cast<uint32_t *>(a.image + l.recordsEnd);
        for (uint32_t i = lane; i < a.metaDirBytes / 4u; i += 64u) mdTo[i] = front(frontWords + i);
    } else {
        const uint64_t *md = reinterpret_cast<const uint64_t *>(a.metaDir);
        uint64_t *mdTo = reinterpret_cast<uint64_t *>(a.image + l.recordsEnd);
        for (uint32_t i = lane; i < a.metaDirBytes / 8u; i += 64u) mdTo[i] = md[i];
    }
    const uint64_t metaDirPos = a.metaDirBytes ? l.recordsEnd + 8u : 0u, tileDirPos = l.tileDirStart + 8u;
    uint32_t headCrc = 0;
    if (a.checksums) {
        // the tile directory's checksum
        const uint64_t nBytes = l.dirSize - 4u, nChunks = (nBytes + GF_FILE_CRC_CHUNK - 1u) / GF_FILE_CRC_CHUNK;
        uint32_t part = 0;
        for (uint64_t c = lane; c < nChunks; c += 64u) {
            const uint64_t end = min(nBytes, (c + 1u) * GF_FILE_CRC_CHUNK);
            part ^= crc_mulmod(crc_xpow8n((uint32_t)(nBytes - end)), a.chunkCrc[c]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) part ^= gf_lane_xor(part, o);
        if (lane == 0u) *reinterpret_cast<uint32_t *>(a.image + l.tileDirStart + nBytes) = part;
        // the header record's: bytes [16, contentPos - 4) with the two positions in place
        const uint32_t *head = reinterpret_cast<const uint32_t *>(a.image + 16u);
        headCrc = wave_crc_words(table, crcWord, lane, [&](uint32_t i) {
            const uint32_t at = 16u + 4u * i;
            if (at == GF_FILE_POS_METADATA_DIR) return (uint32_t)metaDirPos;
            if (at == GF_FILE_POS_METADATA_DIR + 4u) return (uint32_t)(metaDirPos >> 32);
            if (at == GF_FILE_POS_TILE_DIR) return (uint32_t)tileDirPos;
            if (at == GF_FILE_POS_TILE_DIR + 4u) return (uint32_t)(tileDirPos >> 32);
            return IN_ARGS ? front(i) : head[i];
        });
    }
    if (lane == 0u) {
        *reinterpret_cast<uint64_t *>(a.image + GF_FILE_POS_METADATA_DIR) = metaDirPos;
        *reinterpret_cast<uint64_t *>(a.image + GF_FILE_POS_TILE_DIR) = tileDirPos;
        if (IN_ARGS || a.checksums) *reinterpret_cast<uint32_t *>(a.image + a.contentPos - 4u) = headCrc;
    }
    // the file head: "gvrs raster\0", version 1.04, two reserved bytes
    if (lane < 4u) {
        const uint32_t word = lane == 0u ? 0x73727667u : lane == 1u ? 0x73617220u : lane == 2u ? 0x00726574u : 0x00000401u;
        reinterpret_cast<uint32_t *>(a.image)[lane] = word;
    }
}

__global__ __launch_bounds__(64) void k_file_finish(const GfFileWriteArgs a)
{
    __shared__ uint32_t table[256];
    file_finish<false>(a, table, [](uint32_t) { return 0u; });
}

__global__ __launch_bounds__(64) void k_file_finish_front(const GfFileFinishArgs p)
{
    __shared__ uint32_t table[256];
    file_finish<true>(p.a, table, [&](uint32_t i) { return p.front[i]; });
}

}  // namespace

hipError_t gf_launch_file_write(const GfFileWriteArgs &a, const uint8_t *front, hipStream_t stream)
{
    const uint64_t n = (uint64_t)a.nTileRows * (uint64_t)a.nTileCols;
    if (a.nTileRows < 1 || a.nTileCols < 1 || n > 0x7fffffffull) return hipErrorInvalidValue;
    if (((uintptr_t)a.image & 7u) != 0 || (a.firstRecordPos & 7u) != 0 || (a.metaDirBytes & 7u) != 0 || (a.contentPos & 7u) != 0 ||
        a.contentPos < 128u || a.contentPos > a.firstRecordPos)
        return hipErrorInvalidValue;
    const uint64_t frontBytes = a.firstRecordPos - 16u + a.metaDirBytes;
    if (front ? frontBytes > GF_FILE_FRONT_ARG_BYTES : ((uintptr_t)a.metaDir & 7u) != 0) return hipErrorInvalidValue;
    // the largest directory the rectangle of tiles can give: every slot an extended entry
    const uint64_t maxDir = gfFileTileDirSize(n, true), maxChunks = (maxDir + GF_FILE_CRC_CHUNK - 1) / GF_FILE_CRC_CHUNK;
    hipLaunchKernelGGL(k_file_dir_rect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_file_dir_entries, dim3((unsigned)((maxDir / 8 + 255) / 256)), dim3(256), 0, stream, a);
    if (a.checksums) hipLaunchKernelGGL(k_file_dir_crc, dim3((unsigned)((maxChunks + 3) / 4)), dim3(256), 0, stream, a);
    if (front) {
        GfFileFinishArgs p;
        p.a = a;
        memcpy(p.front, front, (size_t)frontBytes);
        memset((uint8_t *)p.front + frontBytes, 0, sizeof(p.front) - (size_t)frontBytes);
        hipLaunchKernelGGL(k_file_finish_front, dim3(1), dim3(64), 0, stream, p);
    } else {
        hipLaunchKernelGGL(k_file_finish, dim3(1), dim3(64), 0, stream, a);
    }
    return hipGetLastError();
}
