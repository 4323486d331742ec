// gvrs_blocks_write.hip -- a block WRITTEN: the rectangle's cells of every element cut into the tiles of the rectangle of tiles, in the
// type the record writer takes, with what the reference's tile cache does on the way (k_block_cut_elems), and the per-tile verdict
// that the record writer receives as its pre-status (k_block_write_verdict); launched by gvrs_api_blocks_write.hip in this order.
// Reference paths are relative to core/src/main/java/org/gridfour/gvrs/: TileElementInt.java:118-126, TileElementShort.java:136-143,
// TileElementFloat.java:133-149, TileElementIntCodedFloat.java:152-169 (setValue / setIntValue: the range checks that throw, the
// float-to-code conversion), TileElement*.hasValidData and RasterTile.java:215-222, RecordManager.java:413-419 (a tile without valid
// data is not written).
//
// The cut moves ROWS with the scheme of gvrs_blocks_common.h: 16-byte stores aligned on the destination, loads before the stores that
// follow them.  Every cell passes through a register on its way, and there it is checked and, for an int-coded float, converted:
// the conversion keeps a cell's four bytes, so it rides on the same pieces.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_blocks_common.h"
#include "gvrs_file_points_store.h"

namespace {

// an element's constants in registers (workgroup-uniform); the cell rule itself -- gf_store_value, gf_store_valid and what they
// are made of -- is gvrs_file_points_store.h, which the writes at scattered points read too
typedef GfStoreElem BwElem;

// One cell on its way: OLD, a cell of the old tile, is only looked at; a cell of the block goes through setValue / setIntValue.
// An out-of-range cell sets GF_BW_FLAG_BOUNDS (the tile gets no record; an ICF's code is then the fill's).
template <int K, bool OLD>
__device__ __forceinline__ uint32_t bw_cell(uint32_t v, const BwElem &p, uint32_t &fl)
{
    uint32_t o = v;
    if (!OLD && !gf_store_value<K>(v, p, o)) fl |= GF_BW_FLAG_BOUNDS;
    if (gf_store_valid<K>(o, p)) fl |= GF_BW_FLAG_VALID;
    return o;
}

// a word of the row: one cell, or two SHORT cells
template <int K, bool OLD>
__device__ __forceinline__ uint32_t bw_word(uint32_t w, const BwElem &p, uint32_t &fl)
{
    if (K == GF_K_ELEM_SHORT) return bw_cell<K, OLD>(w & 0xffffu, p, fl) | (bw_cell<K, OLD>(w >> 16, p, fl) << 16);
    return bw_cell<K, OLD>(w, p, fl);
}

template <int K, bool OLD>
__device__ __forceinline__ GfU4 bw_piece(GfU4 v, const BwElem &p, uint32_t &fl)
{
    v.x = bw_word<K, OLD>(v.x, p, fl), v.y = bw_word<K, OLD>(v.y, p, fl), v.z = bw_word<K, OLD>(v.z, p, fl), v.w = bw_word<K, OLD>(v.w, p, fl);
    return v;
}
template <int K, bool OLD>
__device__ __forceinline__ uint16_t bw_piece(uint16_t v, const BwElem &p, uint32_t &fl)
{
    return (uint16_t)bw_cell<K, OLD>(v, p, fl);
}

// blk_pieces with every piece looked at between its load and its store
template <class T, int K, bool OLD>
__device__ __forceinline__ void bw_pieces(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nPieces, uint32_t l, uint32_t L,
                                          const BwElem &e, uint32_t &fl)
{
    T *__restrict__ d = reinterpret_cast<T *>(dst);
    const T *__restrict__ s = reinterpret_cast<const T *>(src);
#pragma unroll 1
    for (uint32_t p = l; p < nPieces; p += 4u * L) {
        const uint32_t p1 = p + L, p2 = p + 2u * L, p3 = p + 3u * L;
        T v0 = s[p], v1 = v0, v2 = v0, v3 = v0;
        if (p1 < nPieces) v1 = s[p1];
        if (p2 < nPieces) v2 = s[p2];
        if (p3 < nPieces) v3 = s[p3];
        d[p] = bw_piece<K, OLD>(v0, e, fl);
        if (p1 < nPieces) d[p1] = bw_piece<K, OLD>(v1, e, fl);
        if (p2 < nPieces) d[p2] = bw_piece<K, OLD>(v2, e, fl);
        if (p3 < nPieces) d[p3] = bw_piece<K, OLD>(v3, e, fl);
    }
}

// blk_row<false> for the cells of element kind K: one row run of nBytes from src (the block, or the old tile: OLD) to dst
template <int K, bool OLD>
__device__ __forceinline__ void bw_row(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nBytes, const BwElem &e, uint32_t &fl,
                                       uint32_t l, uint32_t L)
{
    constexpr uint32_t item = K == GF_K_ELEM_SHORT ? 2u : 4u;
    if (nBytes == 0u) return;
    const uint32_t diff = (uint32_t)((uintptr_t)dst - (uintptr_t)src);
    const uint32_t unit = (item == 4u || (diff & 3u) == 0u) ? 16u : 2u;
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & (unit - 1u);
    if (head > nBytes) head = nBytes;
    const uint32_t nBody = (nBytes - head) / unit, tail0 = head + nBody * unit;
    const bool hasHead = l * item < head, hasTail = tail0 + l * item < nBytes;
    uint32_t hv = 0, tv = 0;
    if (hasHead) hv = blk_cell_load<false>(src, l * item, item, 0u);
    if (hasTail) tv = blk_cell_load<false>(src, tail0 + l * item, item, 0u);
    if (unit == 16u) bw_pieces<GfU4, K, OLD>(dst + head, src + head, nBody, l, L, e, fl);
    else bw_pieces<uint16_t, K, OLD>(dst + head, src + head, nBody, l, L, e, fl);
    if (hasHead) blk_cell_store(dst, l * item, item, bw_cell<K, OLD>(hv, e, fl));
    if (hasTail) blk_cell_store(dst, tail0 + l * item, item, bw_cell<K, OLD>(tv, e, fl));
}

// the cells of a tile row outside the rectangle: the old tile's, or fill (which is never data)
template <int K>
__device__ __forceinline__ void bw_outside(uint8_t *__restrict__ dst, const uint8_t *__restrict__ old, uint32_t nBytes, const BwElem &e, uint32_t fillWord,
                                           uint32_t &fl, uint32_t l, uint32_t L)
{
    constexpr uint32_t item = K == GF_K_ELEM_SHORT ? 2u : 4u;
    if (old) bw_row<K, true>(dst, old, nBytes, e, fl, l, L);
    else blk_row<true>(dst, nullptr, nBytes, item, fillWord, l, L);
}

// one (element, tile of the rectangle of tiles); returns the lane's flags
template <int K>
__device__ __forceinline__ uint32_t bw_tile(const GfBlockCutElemsArgs &a, const GfBlockCutElem &d, size_t k)
{
    constexpr uint32_t item = K == GF_K_ELEM_SHORT ? 2u : 4u;
    const BwElem e = gf_store_elem(K, d.fillBits, d.fillFBits, d.minBits, d.maxBits, d.scale, d.offset);
    const uint32_t fillWord = blk_fill_word(d.fillBits, item);
    const int64_t ty = (int64_t)(k / (size_t)a.g.nTileCols), tx = (int64_t)(k - (size_t)ty * (size_t)a.g.nTileCols);
    const int64_t gr0 = (a.g.tileRow0 + ty) * a.g.nRowsTile, gc0 = (a.g.tileCol0 + tx) * a.g.nColsTile;   // the tile's first cell on the grid
    const int64_t c0 = blk_max(gc0, (int64_t)a.g.col0), c1 = blk_min(gc0 + a.g.nColsTile, (int64_t)a.g.col0 + a.g.nCols);
    const int64_t r0 = blk_max(gr0, (int64_t)a.g.row0), r1 = blk_min(gr0 + a.g.nRowsTile, (int64_t)a.g.row0 + a.g.nRows);
    const bool touches = c1 > c0 && r1 > r0;                                   // (always: it is a tile of the rectangle of tiles)
    const uint32_t ca = touches ? (uint32_t)(c0 - gc0) : 0u, cb = touches ? (uint32_t)(c1 - gc0) : 0u;
    const uint32_t ra = touches ? (uint32_t)(r0 - gr0) : 0u, rb = touches ? (uint32_t)(r1 - gr0) : 0u;
    const uint32_t nC = (uint32_t)a.g.nColsTile, nR = (uint32_t)a.g.nRowsTile;
    const size_t cells = (size_t)nR * nC, rowBytes = (size_t)nC * item, srcStride = (size_t)a.g.nCols * item;
    uint8_t *__restrict__ tile = reinterpret_cast<uint8_t *>(d.tiles) + k * cells * item;
    const uint8_t *__restrict__ src = reinterpret_cast<const uint8_t *>(d.block) +
                                      (touches ? ((size_t)(r0 - a.g.row0) * (size_t)a.g.nCols + (size_t)(c0 - a.g.col0)) * item : 0);
    const int32_t slot = a.slots ? a.slots[k] : -1;
    const uint8_t *__restrict__ old = slot >= 0 && d.oldTiles ? reinterpret_cast<const uint8_t *>(d.oldTiles) + (size_t)slot * cells * item : nullptr;
    const uint32_t sh = blk_row_lanes_log2((uint32_t)rowBytes), L = 1u << sh, l = threadIdx.x & (L - 1u), step = BLK_THREADS >> sh;
    uint32_t fl = 0;
#pragma unroll 1
    for (uint32_t r = threadIdx.x >> sh; r < nR; r += step) {
        uint8_t *__restrict__ row = tile + (size_t)r * rowBytes;
        const uint8_t *__restrict__ oldRow = old ? old + (size_t)r * rowBytes : nullptr;
        if (r < ra || r >= rb) {
            bw_outside<K>(row, oldRow, (uint32_t)rowBytes, e, fillWord, fl, l, L);
            continue;
        }
        bw_row<K, false>(row + (size_t)ca * item, src + (size_t)(r - ra) * srcStride, (cb - ca) * item, e, fl, l, L);
        bw_outside<K>(row, oldRow, ca * item, e, fillWord, fl, l, L);
        bw_outside<K>(row + (size_t)cb * item, oldRow ? oldRow + (size_t)cb * item : nullptr, (nC - cb) * item, e, fillWord, fl, l, L);
    }
    return fl;
}

// ------------------------------------------------------------------------------------------------
// k_block_cut_elems: a workgroup per (element, tile of the rectangle of tiles), driven by the element table as k_block_gather is (here it travels in the
// kernel arguments).
// Of every tile row the cells whose grid coordinate lies inside the rectangle come from the element's block, checked against the
// element's range and, for an int-coded float, converted to their code; the cells to their left and right, the rows above and
// below and whatever lies beyond the grid are the old tile's where the slot table names an old record, else fill.  Every cell of
// the tile is written exactly once.  Each lane collects "a cell was out of range" and "a cell is not fill" (the kept old cells
// too); a ballot joins them per wave and lane 0 of a wave that saw either issues ONE atomicOr into the tile's flags word.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK_THREADS, 8) void k_block_cut_elems(const GfBlockCutElemsArgs a)
{
    const size_t nRect = (size_t)a.g.nTileRows * (size_t)a.g.nTileCols;
    GF_FOR_WG_TILE(w, (size_t)a.nElems * nRect)
    {
        const size_t ei = w / nRect, k = w - ei * nRect;
        const GfBlockCutElem &d = a.elems[ei];                                 // (kernel arguments, workgroup-uniform: scalar loads)
        uint32_t fl;
        if (d.type == GF_K_ELEM_INT) fl = bw_tile<GF_K_ELEM_INT>(a, d, k);
        else if (d.type == GF_K_ELEM_SHORT) fl = bw_tile<GF_K_ELEM_SHORT>(a, d, k);
        else if (d.type == GF_K_ELEM_FLOAT) fl = bw_tile<GF_K_ELEM_FLOAT>(a, d, k);
        else fl = bw_tile<GF_K_ELEM_ICF>(a, d, k);
        const uint32_t wave = (__ballot((fl & GF_BW_FLAG_BOUNDS) != 0u) ? GF_BW_FLAG_BOUNDS : 0u) |
                              (__ballot((fl & GF_BW_FLAG_VALID) != 0u) ? GF_BW_FLAG_VALID : 0u);
        if ((threadIdx.x & 63u) == 0u && wave) atomicOr(a.flags + k, wave);
    }
}

// ------------------------------------------------------------------------------------------------
// k_block_write_verdict: a lane per tile of the rectangle of tiles.  What the tile gets in place of a record, first match: the
// status of the first element (element order) of its winning old record that is not GF_K_OK, when the rectangle covers the tile
// only partly (the reference would have thrown while reading it); GF_K_ERR_BOUNDS, a cell out of range; GF_K_DECLINED, no element
// has a cell that is not fill (RecordManager.writeTile writes nothing); else 0 and the record writer decides.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK_THREADS) void k_block_write_verdict(const GfBlockWriteVerdictArgs a)
{
    const size_t nRect = (size_t)a.g.nTileRows * (size_t)a.g.nTileCols;
    const size_t k = (size_t)blockIdx.x * BLK_THREADS + threadIdx.x;
    if (k >= nRect) return;
    const int64_t ty = (int64_t)(k / (size_t)a.g.nTileCols), tx = (int64_t)(k - (size_t)ty * (size_t)a.g.nTileCols);
    const int64_t gr0 = (a.g.tileRow0 + ty) * a.g.nRowsTile, gc0 = (a.g.tileCol0 + tx) * a.g.nColsTile;
    const bool whole = gr0 >= a.g.row0 && gc0 >= a.g.col0 && gr0 + a.g.nRowsTile <= (int64_t)a.g.row0 + a.g.nRows &&
                       gc0 + a.g.nColsTile <= (int64_t)a.g.col0 + a.g.nCols;
    int32_t st = 0;
    const int32_t slot = a.slots ? a.slots[k] : -1;
    if (slot >= 0 && !whole)
        for (int e = 0; e < a.nElems && st == 0; e++) st = a.oldStatus[(size_t)e * a.nOld + (size_t)slot];   // (GF_K_OK = 0)
    const uint32_t fl = a.flags[k];
    if (st == 0) st = (fl & GF_BW_FLAG_BOUNDS) ? GF_K_ERR_BOUNDS : (fl & GF_BW_FLAG_VALID) ? 0 : GF_K_DECLINED;
    a.preStatus[k] = st;
    a.tileIndices[k] = (int32_t)((a.g.tileRow0 + ty) * a.g.nColsOfTiles + (a.g.tileCol0 + tx));
}

}  // namespace

hipError_t gf_launch_block_cut_elems(const GfBlockCutElemsArgs &a, hipStream_t stream)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_block_cut_elems, gf_tile_grid((size_t)a.nElems * (size_t)a.g.nTileRows * (size_t)a.g.nTileCols), dim3(BLK_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_block_write_verdict(const GfBlockWriteVerdictArgs &a, hipStream_t stream)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS) return hipErrorInvalidValue;
    const size_t nRect = (size_t)a.g.nTileRows * (size_t)a.g.nTileCols;
    hipLaunchKernelGGL(k_block_write_verdict, dim3((unsigned)((nRect + BLK_THREADS - 1) / BLK_THREADS)), dim3(BLK_THREADS), 0, stream, a);
    return hipGetLastError();
}
