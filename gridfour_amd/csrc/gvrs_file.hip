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
// k_file_locate: a lane per tile of the block's rectangle of tiles, slot j = row-major.  The lanes of a wave run along a tile row,
// so their directory entries are neighbours: one coalesced 4- or 8-byte load each (the entries start at a multiple of 8 of an
// 8-byte aligned image).  A position is judged BEFORE anything is read there: at least contentPos + 8 (a record's content lies
// behind its 8-byte head, and no record lies in the header), a multiple of 8, and position + 12 <= imageBytes (size word, type,
// tile index) -- else GF_K_ERR_BOUNDS and nothing of the tile is read.  An entry that itself lies outside the image is
// GF_K_ERR_BOUNDS too.  Then the record head in one 16-byte load at position - 8 (8-byte aligned; it ends at position + 8, inside
// the image): the tile-index word must be the slot's tile index, else GF_K_ERR_FORMAT -- a directory whose entry leads to another
// tile's record, or to no record at all.  The size word is NOT judged here: the extent [position - 8, min(imageBytes, position
// - 8 + size)) goes to the framing walk, which refuses a size that is too small, no multiple of 8 or longer than its extent, and
// judges the type byte.  Every slot gets an extent (the empty one unless located), a verdict and its present flag: the list
// stays dense, nothing is compacted and the host learns nothing from this kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_file_locate(const GfFileLocateArgs a)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint32_t)a.nTileRows * (uint32_t)a.nTileCols) return;
    const int32_t ty = (int32_t)(j / (uint32_t)a.nTileCols), tx = (int32_t)(j - (uint32_t)ty * (uint32_t)a.nTileCols);
    const int32_t tileRow = a.tileRow0 + ty, tileCol = a.tileCol0 + tx;
    const int32_t tileIndex = tileRow * a.nColsOfTiles + tileCol;                     // (< the grid's tiles <= 0x7fffffff)
    const int32_t dr = tileRow - a.dirRow0, dc = tileCol - a.dirCol0;
    uint64_t start = 0, end = 0;
    int32_t verdict = GF_K_OK;
    uint8_t present = 0;
    if (dr >= 0 && dr < a.dirNRows && dc >= 0 && dc < a.dirNCols) {
        const uint64_t w = a.extended ? 8u : 4u, at = a.entriesPos + ((uint64_t)dr * (uint64_t)a.dirNCols + (uint64_t)dc) * w;
        if (at > a.imageBytes || w > a.imageBytes - at) verdict = GF_K_ERR_BOUNDS;
        else {
            const uint64_t p = a.extended ? *reinterpret_cast<const uint64_t *>(a.image + at)
                                          : (uint64_t) * reinterpret_cast<const uint32_t *>(a.image + at) * 8u;
            if (p != 0) {
                present = 1;
                if (p < a.contentPos + 8u || (p & 7u) != 0u || p > a.imageBytes || a.imageBytes - p < 12u) verdict = GF_K_ERR_BOUNDS;
                else {
                    const GfU4 h = *reinterpret_cast<const GfU4 *>(a.image + (p - 8u));
                    if ((int32_t)h.z != tileIndex) verdict = GF_K_ERR_FORMAT;
                    else {
                        const uint64_t e = (p - 8u) + (uint64_t)h.x;
                        start = p - 8u;
                        end = e < a.imageBytes ? e : a.imageBytes;
                        verdict = GF_FILE_LOCATED;
                    }
                }
            }
        }
    }
    a.starts[j] = start;
    a.ends[j] = end;
    a.verdict[j] = verdict;
    if (a.present) a.present[j] = present;
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
    const uint64_t n = (uint64_t)a.nTileRows * (uint64_t)a.nTileCols;
    if (a.nTileRows < 1 || a.nTileCols < 1 || n > 0x7fffffffull || a.nColsOfTiles < 1) return hipErrorInvalidValue;
    if (((uintptr_t)a.image & 7u) != 0 || (a.entriesPos & 7u) != 0) return hipErrorInvalidValue;
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
