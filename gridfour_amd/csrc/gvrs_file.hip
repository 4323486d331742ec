// gvrs_file.hip -- a GVRS file image in device memory: the tile directory read where it lies (k_file_locate) and the verdicts on
// its entries put into the statuses of a block read (k_file_status), in the order in which gvrs_api_file.hip launches them around
// the records' pipeline (gvrs_records.hip), which runs untouched.
// Reference: gvrs/RecordManager.java:835-856 (readTileDirectory), gvrs/TileDirectory.java:200-257 (compact entries: the position
// divided by 8 as an unsigned int32), gvrs/TileDirectoryExtended.java (int64 positions), gvrs/RecordManager.java:472-520, 746-748
// (readTile seeks to the position: the tile-index word; the size word lies 8 bytes in front of it).

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// k_file_locate: a lane per tile of the block's rectangle of tiles, slot j = row-major, or per tile of a list in ascending order
// (the tiles that a set of points touches: gvrs_file_points.hip).  The lanes of a wave run along a tile row,
// so their directory entries are neighbours: one coalesced 4- or 8-byte load each (the entries start at a multiple of 8 of an
// 8-byte aligned image).  The tile is looked up by gfFileLocateHead (gvrs_file_parse.h), the head in one 16-byte load; a tile
// that is present and passes is GF_FILE_LOCATED.  The size word is not judged here: the extent [position - 8, min(imageBytes,
// position - 8 + size)) goes to the framing walk, which refuses a size that is too small, no multiple of 8 or longer than its
// extent, and judges the type byte.  Every slot gets an extent (the empty one unless located), a verdict and its present flag: the
// list stays dense, nothing is compacted and the host learns nothing from this kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_locate(const GfFileLocateArgs a)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    int32_t tileRow, tileCol;
    if (a.tileList) {                                                                  // (uniform) slot j = the list's tile j
        if (j >= a.nList) return;
        const int32_t t = a.tileList[j];
        tileRow = t / a.dir.nColsOfTiles, tileCol = t - tileRow * a.dir.nColsOfTiles;
    } else {
        if (j >= (uint32_t)a.nTileRows * (uint32_t)a.nTileCols) return;
        const int32_t ty = (int32_t)(j / (uint32_t)a.nTileCols), tx = (int32_t)(j - (uint32_t)ty * (uint32_t)a.nTileCols);
        tileRow = a.tileRow0 + ty, tileCol = a.tileCol0 + tx;
    }
    const int32_t tileIndex = tileRow * a.dir.nColsOfTiles + tileCol;                 // (< the grid's tiles <= 0x7fffffff)
    uint64_t p, start = 0, end = 0;
    GfU4 h;
    int32_t verdict = gfFileLocateHead(a.dir, a.imageBytes, gfDirEntryAt(a.dir, tileRow, tileCol), tileIndex, &p, &h, GfLoadAligned{a.image});
    if (verdict == GF_K_OK && p != 0) {
        const uint64_t e = (p - 8u) + (uint64_t)h.x;
        start = p - 8u;
        end = e < a.imageBytes ? e : a.imageBytes;
        verdict = GF_FILE_LOCATED;
    }
    a.starts[j] = start;
    a.ends[j] = end;
    a.verdict[j] = verdict;
    if (a.present) a.present[j] = p != 0;
}

// ------------------------------------------------------------------------------------------------
// k_file_status: a lane per element instance, behind the records' pipeline.  The framing walk gave the empty extents
// GF_K_ERR_BOUNDS; here a slot that is not located takes its verdict for every element: GF_K_OK for a tile the file does not
// hold (its cells are fill: no record placed anything in its slot of the gather), the refusal otherwise.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_status(const int32_t *__restrict__ verdict, int32_t *__restrict__ status, size_t nSlots, size_t nInst)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= nInst) return;
    const int32_t v = verdict[i % nSlots];
    if (v != GF_FILE_LOCATED) status[i] = v;
}

}  // namespace

hipError_t gf_launch_file_locate(const GfFileLocateArgs &a, hipStream_t stream)
{
    const uint64_t n = a.tileList ? (uint64_t)a.nList : (uint64_t)a.nTileRows * (uint64_t)a.nTileCols;
    if (a.tileList && n == 0) return hipSuccess;
    if ((!a.tileList && (a.nTileRows < 1 || a.nTileCols < 1)) || n > 0x7fffffffull || a.dir.nColsOfTiles < 1) return hipErrorInvalidValue;
    if (((uintptr_t)a.image & 7u) != 0 || !gfDirEntriesAligned(a.dir)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_file_locate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_file_status(const int32_t *verdict, int32_t *status, size_t nSlots, int nElems, hipStream_t stream)
{
    const size_t nInst = nSlots * (size_t)nElems;
    if (nInst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_file_status, dim3((unsigned)((nInst + 255) / 256)), dim3(256), 0, stream, verdict, status, nSlots, nInst);
    return hipGetLastError();
}
