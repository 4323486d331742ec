// gvrs_blocks.hip -- grid blocks in device memory: a rectangle of the raster gathered from decoded tiles (k_block_slots,
// k_block_gather) and a raster cut into tiles (k_grid_cut), in the order in which gvrs_api_blocks.hip launches them.
// The reference assembles a block tile by tile, row by row (gvrs/GvrsElement.java:348-402); tile index and the rectangle of tiles
// a block touches are gvrs/TileAccessIndices.java:79-88, tiles across and down gvrs/GvrsFileSpecification.java:423-424.
//
// All three kernels move ROWS: a tile row's share of the block is one contiguous run of cells on both sides.  Lanes run along
// the row and every store instruction leaves the wave as row pieces (DESIGN section 8 on requests); loads are issued before the
// stores that follow them.  Cells move as bits.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_blocks_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// k_block_slots: a lane per record.  The record's tile index, when it names a tile of the grid inside the block's rectangle of
// tiles, puts the record's number into that tile's slot with atomicMax: of two records of one tile the later one wins, whatever
// the timing.  The table was pre-set to -1; negative indices, indices beyond the grid and tiles outside the rectangle place nothing.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK_THREADS) void k_block_slots(const GfBlockSlotsArgs a)
{
    const size_t t = (size_t)blockIdx.x * BLK_THREADS + threadIdx.x;
    if (t >= a.nRecords) return;
    const int32_t idx = a.tileIndices[t];
    if (idx < 0 || idx >= a.g.nTilesGrid) return;
    const int32_t tr = idx / a.g.nColsOfTiles - a.g.tileRow0, tc = idx % a.g.nColsOfTiles - a.g.tileCol0;
    if (tr < 0 || tr >= a.g.nTileRows || tc < 0 || tc >= a.g.nTileCols) return;
    atomicMax(a.slots + ((size_t)tr * (size_t)a.g.nTileCols + (size_t)tc), (int32_t)t);
}

// ------------------------------------------------------------------------------------------------
// k_block_gather: a workgroup per (element, tile of the block's rectangle of tiles), driven by the slot table.  Rows tr0..tr1,
// columns tc0..tc1 of the tile -- its intersection with the rectangle -- go to their place in the block; where the slot is -1 or
// the element's status of the winning record is not GF_K_OK the fill value goes there instead.  The intersections partition the
// block: every cell is written exactly once, and there is no pre-fill pass.  A row group of L lanes takes a row; the workgroup's
// 256 / L row groups step down the rows, and a row wider than four pieces per lane is looped over (blk_pieces).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK_THREADS, 8) void k_block_gather(const GfBlockGatherArgs a)
{
    const size_t nRect = (size_t)a.g.nTileRows * (size_t)a.g.nTileCols;
    GF_FOR_WG_TILE(w, (size_t)a.nElems * nRect)
    {
        const size_t e = w / nRect, k = w - e * nRect;
        const GfBlockElem d = a.elems ? a.elems[e] : a.one;                    // (workgroup-uniform: scalar loads)
        const int64_t ty = (int64_t)(k / (size_t)a.g.nTileCols), tx = (int64_t)(k - (size_t)ty * (size_t)a.g.nTileCols);
        const int64_t gr0 = (a.g.tileRow0 + ty) * a.g.nRowsTile, gc0 = (a.g.tileCol0 + tx) * a.g.nColsTile;   // the tile's first cell on the grid
        const int64_t r0 = blk_max(gr0, (int64_t)a.g.row0), r1 = blk_min(gr0 + a.g.nRowsTile, (int64_t)a.g.row0 + a.g.nRows);   // [r0, r1) x [c0, c1) on the grid
        const int64_t c0 = blk_max(gc0, (int64_t)a.g.col0), c1 = blk_min(gc0 + a.g.nColsTile, (int64_t)a.g.col0 + a.g.nCols);
        if (r1 <= r0 || c1 <= c0) continue;                                    // (cannot happen: the tile touches the rectangle)
        const uint32_t item = d.itemBytes, runBytes = (uint32_t)(c1 - c0) * item, nRows = (uint32_t)(r1 - r0);
        const uint32_t fillWord = blk_fill_word(d.fillBits, item);
        int32_t slot = a.slots[k];
        if (slot >= 0 && d.status && d.status[slot] != GF_K_OK) slot = -1;
        const size_t cells = (size_t)a.g.nRowsTile * (size_t)a.g.nColsTile;
        const size_t dstStride = (size_t)a.g.nCols * item, srcStride = (size_t)a.g.nColsTile * item;
        uint8_t *__restrict__ dst = reinterpret_cast<uint8_t *>(d.block) + ((size_t)(r0 - a.g.row0) * (size_t)a.g.nCols + (size_t)(c0 - a.g.col0)) * item;
        const uint8_t *__restrict__ src = reinterpret_cast<const uint8_t *>(d.tiles) +
                                          ((size_t)(slot < 0 ? 0 : slot) * cells + (size_t)(r0 - gr0) * (size_t)a.g.nColsTile + (size_t)(c0 - gc0)) * item;
        const uint32_t sh = blk_row_lanes_log2(runBytes), L = 1u << sh, l = threadIdx.x & (L - 1u), step = BLK_THREADS >> sh;
        if (slot < 0) {
#pragma unroll 1
            for (uint32_t r = threadIdx.x >> sh; r < nRows; r += step) blk_row<true>(dst + (size_t)r * dstStride, nullptr, runBytes, item, fillWord, l, L);
        } else {
#pragma unroll 1
            for (uint32_t r = threadIdx.x >> sh; r < nRows; r += step)
                blk_row<false>(dst + (size_t)r * dstStride, src + (size_t)r * srcStride, runBytes, item, fillWord, l, L);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_grid_cut: a workgroup per listed tile, the inverse.  Of every tile row the cells whose grid coordinate lies inside the
// rectangle come from the source raster (row-major nRows x nCols); the cells to their left and right, the rows above and below
// and whatever lies beyond the grid take the fill value, or are left as they are (keepOutside).  A listed index outside the
// grid's tiles: GF_K_ERR_BOUNDS and nothing written.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK_THREADS, 8) void k_grid_cut(const GfGridCutArgs a)
{
    GF_FOR_WG_TILE(j, a.nTiles)
    {
        const int32_t idx = a.tileIndices[j];
        const bool inGrid = idx >= 0 && idx < a.g.nTilesGrid;
        if (threadIdx.x == 0 && a.status) a.status[j] = inGrid ? GF_K_OK : GF_K_ERR_BOUNDS;
        if (!inGrid) continue;
        const uint32_t item = a.itemBytes, fillWord = blk_fill_word(a.fillBits, item);
        const int64_t gr0 = (int64_t)(idx / a.g.nColsOfTiles) * a.g.nRowsTile, gc0 = (int64_t)(idx % a.g.nColsOfTiles) * a.g.nColsTile;
        // the tile's columns [ca, cb) lie inside the rectangle (empty: ca == cb == 0), its rows [ra, rb)
        const int64_t c0 = blk_max(gc0, (int64_t)a.g.col0), c1 = blk_min(gc0 + a.g.nColsTile, (int64_t)a.g.col0 + a.g.nCols);
        const int64_t r0 = blk_max(gr0, (int64_t)a.g.row0), r1 = blk_min(gr0 + a.g.nRowsTile, (int64_t)a.g.row0 + a.g.nRows);
        const bool touches = c1 > c0 && r1 > r0;
        const uint32_t ca = touches ? (uint32_t)(c0 - gc0) : 0u, cb = touches ? (uint32_t)(c1 - gc0) : 0u;
        const uint32_t ra = touches ? (uint32_t)(r0 - gr0) : 0u, rb = touches ? (uint32_t)(r1 - gr0) : 0u;
        const uint32_t nC = (uint32_t)a.g.nColsTile, nR = (uint32_t)a.g.nRowsTile;
        const size_t cells = (size_t)nR * nC, rowBytes = (size_t)nC * item, srcStride = (size_t)a.g.nCols * item;
        uint8_t *__restrict__ tile = reinterpret_cast<uint8_t *>(a.tiles) + j * cells * item;
        // the source cell of the tile's cell (ra, ca)
        const uint8_t *__restrict__ src = reinterpret_cast<const uint8_t *>(a.block) +
                                          (touches ? ((size_t)(r0 - a.g.row0) * (size_t)a.g.nCols + (size_t)(c0 - a.g.col0)) * item : 0);
        const uint32_t sh = blk_row_lanes_log2((uint32_t)rowBytes), L = 1u << sh, l = threadIdx.x & (L - 1u), step = BLK_THREADS >> sh;
        const bool fill = a.keepOutside == 0;
#pragma unroll 1
        for (uint32_t r = threadIdx.x >> sh; r < nR; r += step) {
            uint8_t *__restrict__ row = tile + (size_t)r * rowBytes;
            if (r < ra || r >= rb) {
                if (fill) blk_row<true>(row, nullptr, (uint32_t)rowBytes, item, fillWord, l, L);
                continue;
            }
            blk_row<false>(row + (size_t)ca * item, src + (size_t)(r - ra) * srcStride, (cb - ca) * item, item, fillWord, l, L);
            if (fill) {
                blk_row<true>(row, nullptr, ca * item, item, fillWord, l, L);
                blk_row<true>(row + (size_t)cb * item, nullptr, (nC - cb) * item, item, fillWord, l, L);
            }
        }
    }
}

}  // namespace

hipError_t gf_launch_block_slots(const GfBlockSlotsArgs &a, hipStream_t stream)
{
    if (a.nRecords > 0x7fffffffull) return hipErrorInvalidValue;
    if (a.nRecords == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_slots, dim3((unsigned)((a.nRecords + BLK_THREADS - 1) / BLK_THREADS)), dim3(BLK_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_block_gather(const GfBlockGatherArgs &a, hipStream_t stream)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_block_gather, gf_tile_grid((size_t)a.nElems * (size_t)a.g.nTileRows * (size_t)a.g.nTileCols), dim3(BLK_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_grid_cut(const GfGridCutArgs &a, hipStream_t stream)
{
    if (a.nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_grid_cut, gf_tile_grid(a.nTiles), dim3(BLK_THREADS), 0, stream, a);
    return hipGetLastError();
}
