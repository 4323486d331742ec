// gvrs_file_update.hip -- a GVRS file image UPDATED IN PLACE in device memory: tile records that lie in device memory are placed
// into the image of a file that exists, as GvrsFile(file, "rw") ... close() places them.  gvrs_file_update.h is the host's twin of
// every rule and every byte here (its header has the reference's lines and the one deviation).
//   k_update_snapshot   the old directory's entry of every tile of the grid copied aside (the old directory record is free space)
//   k_update_alloc      ONE wave: the records judged, then the allocator serial over them in the caller's order -- first fit by
//                       ballot over 64 nodes a turn, insert and delete as wave-wide shifts of the position-sorted list, in LDS or
//                       in scratch -- and the three allocations of close.  Writes positions, list and verdict, nothing of the image.
//   k_update_patch      a lane per record: its tile's entry in the copy becomes its new position, or 0
//   k_update_copy       a lane per 8-byte word of the records: to their positions
//   k_update_dir        a lane per 8-byte word of the tile directory's record over the new rectangle, every byte once
//   k_update_dir_crc    a wave per chunk of GF_FILE_CRC_CHUNK bytes of it (both: gvrs_file_dir.h, shared with the write)
//   k_update_fill       a lane per 8-byte word across ALL nodes of the final list: head, zeros, the head's checksum
//   k_update_finish     ONE wave: status and size; the metadata directory, the free-space directory, the tile directory's
//                       checksum folded, time modified, opened-for-writing 0, the three positions and the header's checksum
// Every kernel behind k_update_alloc returns at once unless its verdict is GF_K_OK: an image that does not fit, or whose old
// records are refused, stays byte for byte as it was.  Plain vector stores only; every loop is sized by its arguments.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_file_dir.h"
#include "gvrs_file_update.h"

namespace {

// ------------------------------------------------------------------------------------------------
// k_update_snapshot: a lane per tile of the grid.  grid[t] = the old entry as a position, 0 outside the old rectangle.  The entries
// lie inside the old image: gf_file_update_begin has checked the old directory record against its rectangle.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_snapshot(const GfFileUpdateArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)a.nTilesGrid) return;
    const int64_t k = gfDirEntryOfTile(a.dir, (int32_t)t);
    uint64_t p = 0;
    if (k >= 0) (void)gfDirEntryPos(a.dir, a.oldBytes, (uint64_t)k, &p, GfLoadAligned{a.image});
    a.grid[t] = p;
}

// ---- the list, worked by one wave.  n is wave-uniform; a barrier stands between the loads and the stores of a shift, so that no
// lane's store reaches an element before the lane that moves it has loaded it. ----
struct WaveList {
    uint64_t *pos, *size;
    uint32_t n;
};

__device__ __forceinline__ uint32_t wl_behind(const WaveList &l, uint64_t p, uint32_t lane)      // the first node behind position p
{
    uint32_t k = 0;
    for (uint32_t base = 0; base < l.n; base += 64u) {
        const uint32_t i = base + lane;
        k += (uint32_t)__popcll(__ballot(i < l.n && l.pos[i] <= p));
    }
    return k;
}

__device__ __forceinline__ void wl_erase(WaveList &l, uint32_t k, uint32_t lane)
{
    for (uint32_t base = k + 1u; base < l.n; base += 64u) {
        const uint32_t i = base + lane;
        const bool on = i < l.n;
        uint64_t p = 0, s = 0;
        if (on) p = l.pos[i], s = l.size[i];
        __syncthreads();
        if (on) l.pos[i - 1u] = p, l.size[i - 1u] = s;
        __syncthreads();
    }
    l.n--;
}

__device__ __forceinline__ void wl_insert(WaveList &l, uint32_t k, uint64_t p, uint64_t s, uint32_t lane)
{
    for (uint32_t hi = l.n; hi > k;) {                            // the nodes [k, n) one place up, the highest 64 first
        const uint32_t lo = hi - k > 64u ? hi - 64u : k, i = lo + lane;
        const bool on = i < hi;
        uint64_t q = 0, z = 0;
        if (on) q = l.pos[i], z = l.size[i];
        __syncthreads();
        if (on) l.pos[i + 1u] = q, l.size[i + 1u] = z;
        __syncthreads();
        hi = lo;
    }
    if (lane == 0u) l.pos[k] = p, l.size[k] = s;
    __syncthreads();
    l.n++;
}

__device__ __forceinline__ bool wl_overlaps(const WaveList &l, uint64_t p, uint64_t s, uint32_t lane)
{
    const uint32_t k = wl_behind(l, p, lane);
    return (k > 0u && l.pos[k - 1u] + l.size[k - 1u] > p) || (k < l.n && p + s > l.pos[k]);
}

// fileSpaceDealloc (gfFsDealloc); false: the list is full
__device__ __forceinline__ bool wl_dealloc(WaveList &l, uint32_t cap, uint64_t p, uint64_t s, uint32_t lane)
{
    const uint32_t k = wl_behind(l, p, lane);
    if (k > 0u && l.pos[k - 1u] + l.size[k - 1u] == p) {
        const uint64_t grown = l.size[k - 1u] + s;
        const bool both = k < l.n && l.pos[k - 1u] + grown == l.pos[k];
        const uint64_t all = both ? grown + l.size[k] : grown;
        __syncthreads();
        if (lane == 0u) l.size[k - 1u] = all;
        __syncthreads();
        if (both) wl_erase(l, k, lane);
        return true;
    }
    if (k < l.n && p + s == l.pos[k]) {
        const uint64_t all = l.size[k] + s;
        __syncthreads();
        if (lane == 0u) l.pos[k] = p, l.size[k] = all;
        __syncthreads();
        return true;
    }
    if (l.n >= cap) return false;
    wl_insert(l, k, p, s, lane);
    return true;
}

// fileSpaceAlloc (gfFsAlloc): the record's position.  The list cannot grow: a split puts one node where one was taken.
__device__ __forceinline__ uint64_t wl_alloc(WaveList &l, uint64_t &fileSize, uint64_t sizeToStore, uint32_t lane)
{
    uint32_t k = l.n;
    for (uint32_t base = 0; base < l.n; base += 64u) {
        const uint32_t i = base + lane;
        const uint64_t z = i < l.n ? l.size[i] : 0u;
        const unsigned long long m = __ballot(i < l.n && (z == sizeToStore || z >= sizeToStore + GF_FS_MIN_SPLIT));
        if (m != 0ull) {
            k = base + (uint32_t)__ffsll(m) - 1u;
            break;
        }
    }
    if (k == l.n) {
        if (l.n > 0u && l.pos[l.n - 1u] + l.size[l.n - 1u] == fileSize && l.size[l.n - 1u] < sizeToStore) {
            const uint64_t p = l.pos[l.n - 1u];
            l.n--;
            fileSize = p + sizeToStore;
            return p;
        }
        const uint64_t p = fileSize;
        fileSize += sizeToStore;
        return p;
    }
    const uint64_t p = l.pos[k], surplus = l.size[k] - sizeToStore;
    if (surplus != 0u) {                                          // the surplus takes the node's place: the order by position holds
        __syncthreads();
        if (lane == 0u) l.pos[k] = p + sizeToStore, l.size[k] = surplus;
        __syncthreads();
    } else {
        wl_erase(l, k, lane);
    }
    return p;
}

// ------------------------------------------------------------------------------------------------
// k_update_alloc: ONE wave.  Every value but the lane's share of a ballot or a shift is wave-uniform.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_update_alloc(const GfFileUpdateArgs a)
{
    __shared__ uint64_t lds[2u * GF_UPDATE_LDS_NODES];
    const uint32_t lane = threadIdx.x;
    const bool inLds = a.listCap <= GF_UPDATE_LDS_NODES;
    WaveList l;
    l.pos = inLds ? lds : a.listPos;
    l.size = inLds ? lds + GF_UPDATE_LDS_NODES : a.listSize;
    l.n = a.nOpened;
    if (inLds) {
        for (uint32_t i = lane; i < a.nOpened; i += 64u) l.pos[i] = a.listPos[i], l.size[i] = a.listSize[i];
    }
    __syncthreads();
    GfFileUpdateState st{};
    int32_t verdict = GF_K_OK;
    // the records judged, 64 a turn: what the assembler refuses of records and indices, and two records for one tile
    {
        bool bad = false;
        for (uint64_t base = 0; base < a.nRecords; base += 64u) {
            const uint64_t r = base + lane;
            if (r < a.nRecords) {
                const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1u];
                const int32_t t = a.tiles[r];
                if (o1 < o0 || o1 > a.blobBytes || (o0 & 7u) != 0u || t < 0 || t >= a.nTilesGrid) bad = true;
                else {
                    const uint64_t len = o1 - o0;
                    if (len != 0u && ((len & 7u) != 0u || len < 24u || len > 0x7fffffffull)) bad = true;
                    if (atomicAdd(&a.seen[t], 1u) != 0u) bad = true;
                }
            }
        }
        if (__ballot(bad) != 0ull) verdict = GF_K_ERR_ARG;
    }
    uint64_t fileSize = a.oldBytes;
    uint32_t extended = (a.dir.extended || a.forceExtended) ? 1u : 0u;
    const bool oldEmpty = a.dir.nRows == 0 || a.dir.nCols == 0;
    int64_t r0 = oldEmpty ? 0x7fffffff : a.dir.row0, r1 = oldEmpty ? -1 : (int64_t)a.dir.row0 + a.dir.nRows - 1;
    int64_t c0 = oldEmpty ? 0x7fffffff : a.dir.col0, c1 = oldEmpty ? -1 : (int64_t)a.dir.col0 + a.dir.nCols - 1;
    for (uint64_t r = 0; r < a.nRecords && verdict == GF_K_OK; r++) {
        const uint64_t len = a.offsets[r + 1u] - a.offsets[r];
        const int32_t s = a.status ? a.status[r] : len ? GF_K_OK : 1;
        uint64_t place = GF_UPDATE_UNTOUCHED;
        if (s >= 0) {
            const int32_t tile = a.tiles[r];
            uint64_t oldPos, oldSize;                                // (the statuses are the verdicts' numbers)
            verdict = gfFsTileRecord(a.dir, a.oldBytes, tile, &oldPos, &oldSize, GfLoadAligned{a.image});
            if (verdict != GF_K_OK && a.tileStatus) {                 // the block form: the tile's own verdict, and the tile stays
                if (lane == 0u) a.tileStatus[r] = verdict, a.recPos[r] = GF_UPDATE_UNTOUCHED;
                verdict = GF_K_OK;
                continue;
            }
            if (verdict != GF_K_OK) break;
            if (len != 0u && !a.compression && oldPos != 0u) {       // rewritten where it lies
                if (len != oldSize) verdict = GF_K_ERR_ARG;
                place = oldPos;
            } else {
                if (oldPos != 0u) {
                    if (wl_overlaps(l, oldPos - 8u, oldSize, lane) || !wl_dealloc(l, a.listCap, oldPos - 8u, oldSize, lane)) verdict = GF_K_ERR_FORMAT;
                }
                if (verdict == GF_K_OK) {
                    if (len == 0u) place = oldPos != 0u ? 0u : GF_UPDATE_UNTOUCHED;
                    else {
                        place = wl_alloc(l, fileSize, len, lane) + 8u;
                        if (place > GF_FILE_MAX_COMPACT_POS) extended = 1u;
                        const int64_t row = tile / a.dir.nColsOfTiles, col = tile % a.dir.nColsOfTiles;
                        r0 = row < r0 ? row : r0, r1 = row > r1 ? row : r1, c0 = col < c0 ? col : c0, c1 = col > c1 ? col : c1;
                    }
                }
            }
        }
        if (lane == 0u) a.recPos[r] = place;
    }
    if (verdict == GF_K_OK) {
        // close: the metadata directory, the tile directory, the free-space directory with its second count
        st.metaDirAt = a.metaDirBytes ? wl_alloc(l, fileSize, a.metaDirBytes, lane) : 0u;
        const bool empty = r1 < 0;
        st.nRows = empty ? 0u : (uint32_t)(r1 - r0 + 1), st.nCols = empty ? 0u : (uint32_t)(c1 - c0 + 1);
        st.row0 = empty ? (uint32_t)a.dir.row0 : (uint32_t)r0, st.col0 = empty ? (uint32_t)a.dir.col0 : (uint32_t)c0;
        st.extended = extended;
        st.tileDirSize = gfFileTileDirSize((uint64_t)st.nRows * st.nCols, extended != 0u);
        if (st.tileDirSize > 0x7fffffffull) verdict = GF_K_ERR_UNSUPPORTED;
        else {
            st.tileDirAt = wl_alloc(l, fileSize, st.tileDirSize, lane);
            st.hasFreeDir = l.n != 0u ? 1u : 0u;
            if (st.hasFreeDir) {
                st.freeDirSize = gfFileRecordSize(4u + 12u * (uint64_t)l.n);
                if (st.freeDirSize > 0x7fffffffull) verdict = GF_K_ERR_UNSUPPORTED;
                else st.freeDirAt = wl_alloc(l, fileSize, st.freeDirSize, lane);
            }
        }
    }
    if (verdict == GF_K_OK) {
        bool big = false;
        for (uint32_t base = 0; base < l.n; base += 64u) big |= base + lane < l.n && l.size[base + lane] > 0x7fffffffull;
        if (__ballot(big) != 0ull) verdict = GF_K_ERR_UNSUPPORTED;
    }
    if (verdict == GF_K_OK) {
        st.total = fileSize;
        st.nFinal = l.n;
        if (fileSize > a.imageCap) verdict = GF_K_ERR_CAPACITY;
        else {
            // the final list and the prefix sums of its sizes, for the kernels behind
            if (inLds)
                for (uint32_t i = lane; i < l.n; i += 64u) a.listPos[i] = l.pos[i], a.listSize[i] = l.size[i];
            __syncthreads();
            if (lane == 0u) {
                uint64_t sum = 0;
                for (uint32_t i = 0; i < l.n; i++) {
                    a.listPrefix[i] = sum;
                    sum += l.size[i];
                }
                a.listPrefix[l.n] = sum;
            }
        }
    }
    st.verdict = verdict;
    if (verdict != GF_K_OK && verdict != GF_K_ERR_CAPACITY) st.total = 0;
    if (lane == 0u) *a.state = st;
}

// ------------------------------------------------------------------------------------------------
// k_update_patch: a lane per record.  No two records name one tile (k_update_alloc has refused that).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_patch(const GfFileUpdateArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (a.state->verdict != GF_K_OK || r >= a.nRecords) return;
    const uint64_t p = a.recPos[r];
    if (p != GF_UPDATE_UNTOUCHED) a.grid[a.tiles[r]] = p;
}

// ------------------------------------------------------------------------------------------------
// k_update_copy: a lane per 8-byte word of the blob [offsets[0], offsets[nRecords]); its record by bisection of the offsets.
// Source and target are 8-byte aligned: offsets, lengths and positions are multiples of 8.  The target [pos - 8, pos - 8 + len)
// lies inside [contentPos, total) and total <= imageCap.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_copy(const GfFileUpdateArgs a)
{
    if (a.state->verdict != GF_K_OK || a.nRecords == 0u) return;
    const uint64_t first = a.offsets[0], b = first + ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 8u;
    if (b >= a.offsets[a.nRecords]) return;
    uint64_t lo = 0, hi = a.nRecords;                             // the last record with offsets[r] <= b
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a.offsets[mid] <= b) lo = mid;
        else hi = mid;
    }
    const uint64_t p = a.recPos[lo];
    if (p == GF_UPDATE_UNTOUCHED || p == 0u || b >= a.offsets[lo + 1u]) return;
    *reinterpret_cast<uint2 *>(a.image + p - 8u + (b - a.offsets[lo])) = *reinterpret_cast<const uint2 *>(a.blob + b);
}

__device__ __forceinline__ GfTileDirRec upd_dir(const GfFileUpdateState &s)
{
    return GfTileDirRec{s.tileDirAt, s.tileDirSize, s.extended, s.row0, s.col0, s.nRows, s.nCols};
}

// ------------------------------------------------------------------------------------------------
// k_update_dir, k_update_dir_crc: as k_file_dir_entries and k_file_dir_crc, over the new rectangle; a tile's entry: its word of
// the grid.  The record's last 4 bytes are left to k_update_finish with checksums.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_dir(const GfFileUpdateArgs a)
{
    const GfFileUpdateState s = *a.state;
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s.verdict != GF_K_OK || w >= s.tileDirSize / 8u) return;
    tile_dir_store_word(a.image, upd_dir(s), w, a.checksums != 0,
                        [&](uint32_t row, uint32_t col) { return a.grid[(uint64_t)row * (uint32_t)a.dir.nColsOfTiles + col]; });
}

__global__ __launch_bounds__(256) void k_update_dir_crc(const GfFileUpdateArgs a)
{
    __shared__ uint32_t table[256];
    crc_table_fill_256(table);
    const GfFileUpdateState s = *a.state;
    if (s.verdict == GF_K_OK) tile_dir_chunk_crc(table, a.image, upd_dir(s), (uint64_t)blockIdx.x * 4u + gf_wave_id(), threadIdx.x & 63u, a.chunkCrc);
}

// ------------------------------------------------------------------------------------------------
// k_update_fill: the lanes stride over the 8-byte words of all free nodes together (one node may be most of the file); a word's
// node by bisection of the prefix sums.  First word: the size and type 0; last word: zero and the head's checksum; else zero.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_fill(const GfFileUpdateArgs a)
{
    const GfFileUpdateState s = *a.state;
    if (s.verdict != GF_K_OK || s.nFinal == 0u) return;
    const uint64_t nWords = a.listPrefix[s.nFinal] / 8u, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < nWords; w += stride) {
        const uint64_t b = w * 8u;
        uint32_t lo = 0, hi = s.nFinal;                           // the last node with prefix[k] <= b
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (a.listPrefix[mid] <= b) lo = mid;
            else hi = mid;
        }
        const uint64_t in = b - a.listPrefix[lo], size = a.listSize[lo];
        uint2 v = make_uint2(0u, 0u);
        if (in == 0u) v.x = (uint32_t)size;
        else if (in == size - 8u && a.checksums) v.y = ~gfCrcWordBits(gfCrcWordBits(0xffffffffu, (uint32_t)size), 0u);   // (of its head)
        *reinterpret_cast<uint2 *>(a.image + a.listPos[lo] + in) = v;
    }
}

// ------------------------------------------------------------------------------------------------
// k_update_finish: ONE wave.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_update_finish(const GfFileUpdateArgs a)
{
    __shared__ uint32_t table[256];
    const uint32_t lane = threadIdx.x;
    crc_table_fill_wave(table, lane);
    const GfFileUpdateState s = *a.state;
    if (lane == 0u) {
        *a.imageBytes = s.total;
        *a.fileStatus = s.verdict;
    }
    if (s.verdict != GF_K_OK) return;
    // the metadata directory: the old record, whole
    {
        const uint64_t *md = reinterpret_cast<const uint64_t *>(a.metaDir);
        uint64_t *to = reinterpret_cast<uint64_t *>(a.image + s.metaDirAt);
        for (uint32_t i = lane; i < a.metaDirBytes / 8u; i += 64u) to[i] = md[i];
    }
    // the free-space directory: [size][3 0 0 0][int32 count]{[int64 position][int32 size]}[zeros][checksum], in 4-byte words
    if (s.hasFreeDir) {
        const uint32_t n4 = (uint32_t)s.freeDirSize / 4u;
        const auto word = [&](uint32_t i) -> uint32_t {
            if (i == 0u) return (uint32_t)s.freeDirSize;
            if (i == 1u) return (uint32_t)GF_FILE_REC_FREE_DIR;
            if (i == 2u) return s.nFinal;
            const uint32_t k = (i - 3u) / 3u, m = (i - 3u) % 3u;
            if (k >= s.nFinal) return 0u;
            return m == 0u ? (uint32_t)a.listPos[k] : m == 1u ? (uint32_t)(a.listPos[k] >> 32) : (uint32_t)a.listSize[k];
        };
        uint32_t *to = reinterpret_cast<uint32_t *>(a.image + s.freeDirAt);
        for (uint32_t i = lane; i < n4 - 1u; i += 64u) to[i] = word(i);
        const uint32_t crc = a.checksums ? wave_crc_words(table, n4 - 1u, lane, word) : 0u;
        if (lane == 0u) to[n4 - 1u] = crc;
    }
    // the header record's fields this kernel computes, for its checksum and for the stores
    const GfHeadField fields[5] = {{(uint32_t)GF_FILE_POS_TIME_MODIFIED, (uint64_t)a.timeModified},
                                   {(uint32_t)GF_FILE_POS_OPENED, 0u},
                                   {(uint32_t)GF_FILE_POS_FREE_DIR, s.hasFreeDir ? s.freeDirAt + 8u : 0u},
                                   {(uint32_t)GF_FILE_POS_METADATA_DIR, a.metaDirBytes ? s.metaDirAt + 8u : 0u},
                                   {(uint32_t)GF_FILE_POS_TILE_DIR, s.tileDirAt + 8u}};
    uint32_t headCrc = 0;
    if (a.checksums) {
        tile_dir_fold(a.image, upd_dir(s), a.chunkCrc, lane);
        // the header record's checksum: bytes [16, contentPos - 4)
        const uint32_t *head = reinterpret_cast<const uint32_t *>(a.image + 16u);
        headCrc = head_crc(table, (uint32_t)(a.dir.contentPos - 16u - 4u) / 4u, lane, fields, [&](uint32_t i) { return head[i]; });
    }
    if (lane == 0u) {
        head_store(a.image, fields);
        if (a.checksums) *reinterpret_cast<uint32_t *>(a.image + a.dir.contentPos - 4u) = headCrc;
    }
}

}  // namespace

hipError_t gf_launch_file_update(const GfFileUpdateArgs &a, hipStream_t stream)
{
    if (((uintptr_t)a.image & 7u) != 0 || ((uintptr_t)a.blob & 7u) != 0 || ((uintptr_t)a.metaDir & 7u) != 0 || (a.metaDirBytes & 7u) != 0 ||
        (a.dir.contentPos & 7u) != 0 || a.dir.contentPos < 128u || a.dir.contentPos > a.oldBytes || a.oldBytes > a.imageCap || (a.oldBytes & 7u) != 0 ||
        a.nTilesGrid < 1 || a.dir.nColsOfTiles < 1 || a.nOpened > a.listCap || a.nRecords > 0x7fffffffull)
        return hipErrorInvalidValue;
    const uint64_t n = (uint64_t)a.nTilesGrid;
    const uint64_t maxDir = gfFileTileDirSize(n, true), maxChunks = (maxDir + GF_FILE_CRC_CHUNK - 1) / GF_FILE_CRC_CHUNK;
    const uint64_t blobWords = a.blobBytes / 8u, capWords = a.imageCap / 8u;
    hipLaunchKernelGGL(k_update_snapshot, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_update_alloc, dim3(1), dim3(64), 0, stream, a);
    if (a.nRecords) {
        hipLaunchKernelGGL(k_update_patch, dim3((unsigned)((a.nRecords + 255) / 256)), dim3(256), 0, stream, a);
        if (blobWords) hipLaunchKernelGGL(k_update_copy, dim3((unsigned)((blobWords + 255) / 256)), dim3(256), 0, stream, a);
    }
    hipLaunchKernelGGL(k_update_dir, dim3((unsigned)((maxDir / 8 + 255) / 256)), dim3(256), 0, stream, a);
    if (a.checksums) hipLaunchKernelGGL(k_update_dir_crc, dim3((unsigned)((maxChunks + 3) / 4)), dim3(256), 0, stream, a);
    // the free nodes lie inside the image: at most imageCap / 8 words, a few to a lane
    hipLaunchKernelGGL(k_update_fill, dim3((unsigned)std::min<uint64_t>(1024u, (capWords + 255) / 256 + 1)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_update_finish, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}
