"""A numpy model of grid blocks, used only by the tests: what the loops of GvrsElement.readBlock compute (gvrs/GvrsElement.java:
348-402, TileAccessIndices.java:79-88) and their inverse.  Tiles are placed by index into a full nRowsOfTiles * tr x
nColsOfTiles * tc array pre-set to the fill value; the rectangle is a slice of it."""
import numpy as np


def tiles_of(grid_shape, tile_shape):
    """(tiles down, tiles across) = ceil(grid / tile) (GvrsFileSpecification.java:423-424)"""
    return -(-grid_shape[0] // tile_shape[0]), -(-grid_shape[1] // tile_shape[1])


def _full(grid_shape, tile_shape, fill, dtype):
    nrt, nct = tiles_of(grid_shape, tile_shape)
    return np.full((nrt * tile_shape[0], nct * tile_shape[1]), fill, dtype)


def block_from_tiles(grid_shape, tile_shape, rect, indices, tiles, fill, ok=None):
    """tiles [n, tr * tc] listed with their tile indices, in list order (of two entries of one tile the later one counts); an
    entry that is not ok leaves fill; indices outside [0, nTiles) place nothing"""
    tiles = np.asarray(tiles)
    tr, tc = tile_shape
    nrt, nct = tiles_of(grid_shape, tile_shape)
    full = _full(grid_shape, tile_shape, fill, tiles.dtype)
    for j, idx in enumerate(indices):
        idx = int(idx)
        if idx < 0 or idx >= nrt * nct:
            continue
        r, c = divmod(idx, nct)
        full[r * tr:(r + 1) * tr, c * tc:(c + 1) * tc] = tiles[j].reshape(tr, tc) if ok is None or ok[j] else fill
    r0, c0, nr, nc = rect
    return full[r0:r0 + nr, c0:c0 + nc].copy()


def tiles_from_block(grid_shape, tile_shape, rect, block, indices, fill, before=None):
    """the inverse: the listed tiles of a raster that holds `block` at rect and fill everywhere else (beyond the grid too);
    before [n, tr * tc]: what the tiles held, kept outside the rectangle (keep_outside).  Every listed index must be valid."""
    block = np.asarray(block)
    tr, tc = tile_shape
    nrt, nct = tiles_of(grid_shape, tile_shape)
    full = _full(grid_shape, tile_shape, fill, block.dtype)
    inside = np.zeros(full.shape, bool)
    r0, c0, nr, nc = rect
    full[r0:r0 + nr, c0:c0 + nc] = block.reshape(nr, nc)
    inside[r0:r0 + nr, c0:c0 + nc] = True
    out = np.empty((len(indices), tr * tc), block.dtype)
    for j, idx in enumerate(indices):
        r, c = divmod(int(idx), nct)
        assert 0 <= int(idx) < nrt * nct
        t = full[r * tr:(r + 1) * tr, c * tc:(c + 1) * tc].reshape(-1)
        if before is not None:
            t = np.where(inside[r * tr:(r + 1) * tr, c * tc:(c + 1) * tc].reshape(-1), t, before[j])
        out[j] = t
    return out
