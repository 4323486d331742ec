// gvrs_file_write.hip -- a GVRS file image finished in device memory, behind the record writer (gvrs_records_enc.hip) that has laid
// the tile records into it: the bounding rectangle of the tiles with a record and the extended decision (k_file_dir_rect), the tile
// directory's record (k_file_dir_entries), its CRC-32C in chunks (k_file_dir_crc), and the rest (k_file_finish): the metadata
// directory copied to its place, the chunks' checksums folded, the two directory positions patched into the header record, its
// checksum, the image's size and status, and last the 16 bytes of the file head; a short front (header and metadata records,
// metadata directory) arrives in its arguments and is written by it too.  The directory's record and the header's computed fields
// are laid by gvrs_file_dir.h, shared with the update (gvrs_file_update.hip).  gvrs_file_emit.h is the host's twin of every
// byte written here and holds GF_FILE_CRC_CHUNK.  Plain vector stores only.
// Reference: gvrs/RecordManager.java:864-883 (writeTileDirectory), :87, 451-454 (the extended decision), gvrs/TileDirectory.java:
// 266-290, gvrs/TileDirectoryExtended.java (writeTilePositions), gvrs/GvrsFile.java:584-616 (close: positions, header checksum).

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_file_dir.h"

namespace {

// What every kernel behind k_file_dir_rect derives from the state it left: the directory's rectangle and form, and where things lie.
struct FileLayout {
    GfTileDirRec dir;                  // the tile directory's record
    uint64_t recordsEnd, total;
    bool fits;                         // total <= imageCap: the records were all written and both directories have room
};

__device__ __forceinline__ FileLayout file_layout(const GfFileWriteArgs &a)
{
    const GfFileWriteState s = *a.state;
    FileLayout l;
    GfTileDirRec &d = l.dir;
    const bool any = s.row1p != 0u;
    d.row0 = any ? ~s.invRow0 : 0u, d.col0 = any ? ~s.invCol0 : 0u;
    d.nRows = any ? s.row1p - d.row0 : 0u, d.nCols = any ? s.col1p - d.col0 : 0u;
    d.extended = (a.forceExtended || s.extended) ? 1u : 0u;
    d.size = gfFileTileDirSize((uint64_t)d.nRows * (uint64_t)d.nCols, d.extended != 0u);
    l.recordsEnd = a.firstRecordPos + a.offsets[(uint64_t)a.nTileRows * (uint64_t)a.nTileCols];
    d.at = l.recordsEnd + a.metaDirBytes;
    l.total = d.at + d.size;
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

// ------------------------------------------------------------------------------------------------
// k_file_dir_entries: a lane per 8-byte word of the directory's record (tile_dir_store_word).  A tile's entry: its slot in the
// rectangle of tiles, 0 for a slot without a record.  Nothing is written when the image does not fit.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_dir_entries(const GfFileWriteArgs a)
{
    const FileLayout l = file_layout(a);
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (!l.fits || w >= l.dir.size / 8u) return;
    tile_dir_store_word(a.image, l.dir, w, a.checksums != 0, [&](uint32_t row, uint32_t col) -> uint64_t {
        const uint64_t j = (uint64_t)(row - (uint32_t)a.tileRow0) * (uint32_t)a.nTileCols + (col - (uint32_t)a.tileCol0);
        const uint64_t o0 = a.offsets[j], o1 = a.offsets[j + 1];
        return o1 != o0 ? a.firstRecordPos + o0 + 8u : 0u;
    });
}

// ------------------------------------------------------------------------------------------------
// k_file_dir_crc: a wave per chunk of the directory's record (tile_dir_chunk_crc), four waves a workgroup around the byte table in
// LDS; k_file_finish folds the chunks' checksums.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_dir_crc(const GfFileWriteArgs a)
{
    __shared__ uint32_t table[256];
    crc_table_fill_256(table);
    const FileLayout l = file_layout(a);
    if (l.fits) tile_dir_chunk_crc(table, a.image, l.dir, (uint64_t)blockIdx.x * 4u + gf_wave_id(), threadIdx.x & 63u, a.chunkCrc);
}

// ------------------------------------------------------------------------------------------------
// k_file_finish: ONE wave.  The image's size and status first.  An image that does not fit gets nothing more than zeros in the
// bytes of the file head that lie in front of imageCap: it does not open.  Else the metadata directory's record goes to its place
// behind the records (8-byte words), the chunks' checksums are folded into the directory's last word (tile_dir_fold), the two
// positions -- the one list `fields` -- go into the header record and its checksum is computed over the record with them in place
// (head_crc), and last the file head.
// IN_ARGS: the front -- the image's bytes [16, firstRecordPos) and the metadata directory -- lies in the kernel's arguments
// (front(i) = its word i) and is written here too, every word but the fields' and the checksum's; else it was copied to the image
// and to a.metaDir before the kernels ran.
// ------------------------------------------------------------------------------------------------
template <bool IN_ARGS, class Front>
__device__ __forceinline__ void file_finish(const GfFileWriteArgs &a, uint32_t *table, Front front)
{
    const uint32_t lane = threadIdx.x;
    crc_table_fill_wave(table, lane);
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
    const GfHeadField fields[2] = {{(uint32_t)GF_FILE_POS_METADATA_DIR, a.metaDirBytes ? l.recordsEnd + 8u : 0u},
                                   {(uint32_t)GF_FILE_POS_TILE_DIR, l.dir.at + 8u}};
    // the header record and the metadata records (the fields and the checksum: below)
    if (IN_ARGS) {
        uint32_t *to = reinterpret_cast<uint32_t *>(a.image + 16u);
        for (uint32_t i = lane; i < frontWords; i += 64u)
            if (!head_computed(fields, 16u + 4u * i) && i != crcWord) to[i] = front(i);
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
    uint32_t headCrc = 0;
    if (a.checksums) {
        tile_dir_fold(a.image, l.dir, a.chunkCrc, lane);
        // the header record's checksum: bytes [16, contentPos - 4)
        const uint32_t *head = reinterpret_cast<const uint32_t *>(a.image + 16u);
        headCrc = head_crc(table, crcWord, lane, fields, [&](uint32_t i) { return IN_ARGS ? front(i) : head[i]; });
    }
    if (lane == 0u) {
        head_store(a.image, fields);
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
