// gvrs_file_points.h -- reads at scattered points of a GVRS file, restated once for host and device: which tile and which cell of
// it a grid cell is (gvrs/TileAccessIndices.java:78-92 computeAccessIndices), which tiles the 4 x 4 window of an interpolation
// point touches (the window is gf_interp_window's, gvrs_interp_common.h: nothing of it is restated here), and where a touched
// tile's decoded cells lie in the pool of a call (its rank among the touched tiles, from a bitmap of one bit per tile of the grid
// and the exclusive prefix of the popcounts of its words).  Used by the kernels of gvrs_file_points.hip, by the host forms of
// gvrs_api_file_points.hip and by a stand-alone CPU program (tests/csrc/file_points_test.cpp).
// Reference paths are relative to core/src/main/java/org/gridfour/.
#pragma once

#include <stdint.h>

#include "gvrs_common.h"
#include "gvrs_interp_common.h"

// the grid as the point reads take it (GvrsFileSpecification.java:423-424 for the tiles across)
struct GfPointsGrid {
    int32_t nRowsGrid, nColsGrid, nRowsTile, nColsTile;
    int32_t nColsOfTiles, nTilesGrid;
};

GF_HD GfPointsGrid gf_points_grid(int32_t nRowsGrid, int32_t nColsGrid, int32_t nRowsTile, int32_t nColsTile)
{
    GfPointsGrid g;
    g.nRowsGrid = nRowsGrid, g.nColsGrid = nColsGrid, g.nRowsTile = nRowsTile, g.nColsTile = nColsTile;
    g.nColsOfTiles = (int32_t)(((int64_t)nColsGrid + nColsTile - 1) / nColsTile);
    g.nTilesGrid = (int32_t)((((int64_t)nRowsGrid + nRowsTile - 1) / nRowsTile) * g.nColsOfTiles);
    return g;
}

// computeAccessIndices (TileAccessIndices.java:78-92): false for a row or column outside the grid (the reference throws)
GF_HD bool gf_points_cell(const GfPointsGrid &g, int32_t row, int32_t col, int32_t &tileIndex, int32_t &indexInTile)
{
    if (row < 0 || row >= g.nRowsGrid || col < 0 || col >= g.nColsGrid) return false;
    const int32_t tileRow = row / g.nRowsTile, tileCol = col / g.nColsTile;
    tileIndex = tileRow * g.nColsOfTiles + tileCol;
    indexInTile = (row - tileRow * g.nRowsTile) * g.nColsTile + (col - tileCol * g.nColsTile);
    return true;
}

// The tiles of a window (row0, col0, n1) that gf_interp_window accepted: rows row0 .. row0 + 3; columns col0 .. col0 + n1 - 1
// followed by columns 0 .. 3 - n1 when it wraps (n1 < 4).  The distinct tiles, in ascending tile index: per tile row the wrapped
// run's tile columns (they begin at 0: nB of them) and then those of the first run that lie behind them (nA from a0 on).  Tiles
// of fewer than 4 cells a side make it up to 4 tile rows and 4 or more tile columns.
struct GfWindowTiles {
    int32_t tr0, nTr, nB, a0, nA, nColsOfTiles;
    GF_HD int32_t count() const { return nTr * (nB + nA); }
    GF_HD int32_t at(int32_t k) const                                          // tile k < count() of the window
    {
        const int32_t nc = nB + nA, r = k / nc, j = k - r * nc;
        return (tr0 + r) * nColsOfTiles + (j < nB ? j : a0 + (j - nB));
    }
};
GF_HD GfWindowTiles gf_points_window_tiles(const GfPointsGrid &g, int32_t row0, int32_t col0, int32_t n1)
{
    GfWindowTiles t;
    t.tr0 = row0 / g.nRowsTile;
    t.nTr = (row0 + 3) / g.nRowsTile - t.tr0 + 1;
    t.nB = n1 < 4 ? (3 - n1) / g.nColsTile + 1 : 0;
    const int32_t a0 = col0 / g.nColsTile, a1 = (col0 + n1 - 1) / g.nColsTile;
    t.a0 = a0 < t.nB ? t.nB : a0;                                              // (a grid of a few columns: the runs share tiles)
    t.nA = a1 >= t.a0 ? a1 - t.a0 + 1 : 0;
    t.nColsOfTiles = g.nColsOfTiles;
    return t;
}

// the grid column of sample k of a window's row
GF_HD int32_t gf_points_window_col(int32_t col0, int32_t n1, int k) { return k < n1 ? col0 + k : k - n1; }

// GfInterpGeom for the whole grid of a file: the block is the grid, so gf_interp_window_in_block holds for every accepted window
GF_HD void gf_points_whole_grid(GfInterpGeom &ig, const GfPointsGrid &g)
{
    ig.nRowsGrid = g.nRowsGrid, ig.nColsGrid = g.nColsGrid;
    ig.bRow0 = 0, ig.bCol0 = 0, ig.bRows = g.nRowsGrid, ig.bCols = g.nColsGrid;
}

// ---- the bitmap of touched tiles: bit (tile & 31) of word (tile >> 5) ----
GF_HD uint32_t gf_points_popcount(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}
GF_HD size_t gf_points_words(int32_t nTilesGrid) { return ((size_t)nTilesGrid + 31u) >> 5; }

// a touched tile's slot: its rank among the touched tiles = where its record lies in the list and its cells in the pool
GF_HD uint32_t gf_points_slot(const uint32_t *bits, const uint32_t *prefix, int32_t tile)
{
    const uint32_t w = (uint32_t)tile >> 5;
    return prefix[w] + gf_points_popcount(bits[w] & ((1u << ((uint32_t)tile & 31u)) - 1u));
}
