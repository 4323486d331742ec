"""A numpy restatement of the reads at points of a GVRS file, written from the reference and independent of the C++: which tile
and which cell of it a grid cell is (gvrs/TileAccessIndices.java:78-92), which tiles the 4 x 4 window of an interpolation point
touches (the window is interp_ref.window, from gvrs/GvrsInterpolatorBSpline.java:374-484), and what a cell read delivers, from a
whole-grid array plus a per-tile status map."""
import numpy as np

import interp_ref as IR

OK, ERR_ARG = 0, -4


def tiles_across(grid):
    return -(-grid[1] // grid[3])


def cell_tiles(grid, rows, cols):
    """(inside [n] bool, tile index [n], index in tile [n]); the last two are 0 for a cell outside the grid"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    inside = (rows >= 0) & (rows < grid[0]) & (cols >= 0) & (cols < grid[1])
    r, c = np.where(inside, rows, 0), np.where(inside, cols, 0)
    tile = (r // grid[2]) * tiles_across(grid) + c // grid[3]
    at = (r % grid[2]) * grid[3] + c % grid[3]
    return inside, np.where(inside, tile, 0), np.where(inside, at, 0)


def cells_touched(grid, rows, cols):
    inside, tile, _ = cell_tiles(grid, rows, cols)
    return np.unique(tile[inside]).astype(np.int32)


def spec_of(grid, wrap=0, row_fringe=None, col_fringe=None, **kw):
    return IR.Spec(grid[0], grid[1], wrap=wrap, row_fringe=row_fringe, col_fringe=col_fringe, **kw)


def window_tiles(grid, spec, rows, cols):
    """per point the sorted list of the distinct tiles of its window; [] for a point without one"""
    status, row0, col0, n1, _, _ = IR.window(spec, rows, cols)
    across = tiles_across(grid)
    out = []
    for s, r0, c0, k1 in zip(status.tolist(), row0.tolist(), col0.tolist(), n1.tolist()):
        if s != IR.OK:
            out.append([])
            continue
        wcols = [c0 + k for k in range(k1)] + list(range(4 - k1))
        out.append(sorted({(r // grid[2]) * across + c // grid[3] for r in range(r0, r0 + 4) for c in wcols}))
    return out


def windows_touched(grid, spec, rows, cols):
    seen = set()
    for t in window_tiles(grid, spec, rows, cols):
        seen.update(t)
    return np.array(sorted(seen), np.int32)


def slots(grid, touched):
    """the bitmap's words, the exclusive prefix of their popcounts, and every touched tile's slot by the kernels' rule"""
    n_tiles = -(-grid[0] // grid[2]) * tiles_across(grid)
    bits = np.zeros((n_tiles + 31) // 32, np.uint32)
    for t in touched:
        bits[t >> 5] |= np.uint32(1 << (t & 31))
    counts = np.array([bin(int(w)).count("1") for w in bits], np.int64)
    prefix = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return bits, prefix, [int(prefix[t >> 5]) + bin(int(bits[t >> 5]) & ((1 << (t & 31)) - 1)).count("1") for t in touched]


def expected_cells(grid, whole, fill, tile_status, rows, cols):
    """(values [n], status [n]) of a cell read of one element: whole = the whole-grid array a block read delivers (fill where a
    tile failed or is absent), tile_status = {tile index: status} for the tiles whose status is not OK"""
    inside, tile, _ = cell_tiles(grid, rows, cols)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    values = np.full(rows.shape, fill, whole.dtype)
    values[inside] = whole[rows[inside], cols[inside]]
    status = np.where(inside, OK, ERR_ARG).astype(np.int32)
    for t, s in tile_status.items():
        hit = inside & (tile == t)
        status[hit] = s
        values[hit] = fill
    return values, status
