"""Test-only model of writes at scattered points into a GVRS file: a plain sequential restatement of
    for i in range(n): for e: element[e].writeValue(rows[i], cols[i], values[e][i])
followed by close(), on top of the cell rule of tests/block_write_ref.py (TileElement*.setValue, hasValidData) and the file model
of tests/gvrs_file_update_ref.py.  The touched tiles are taken in ascending index; a tile's old cells come from the caller's reader
(an int-coded float's as CODES), or are fill for a tile without a record; the points are stored one after the other, so of several
points on one cell the last whose value passed wins; the verdicts follow; the surviving tiles go through the caller's record
writer and the records to the update model in ascending tile index.
Elements are described as GvrsFileHip.elems gives them; fills: per element the fill value, None for an "icf" (its own fill_i)."""
import struct

import numpy as np

import block_write_ref as BW
import gvrs_file_update_ref as R

OK, DECLINED, ERR_FORMAT, ERR_BOUNDS, ERR_ARG, ERR_CAPACITY = 0, 1, -1, -2, -4, -5


def fills_of(info):
    """GvrsFileHip.info -> the fills as this model takes them"""
    out = []
    for el in info["elems"]:
        out.append(None if el["type"] == 3 else (el["fill_f"] if el["type"] == 2 else el["fill_i"]))
    return out


def tiles_of(grid):
    return -(-grid[0] // grid[2]), -(-grid[1] // grid[3])


def cell_of(grid, row, col):
    """TileAccessIndices.computeAccessIndices -> (tile, index in tile), None outside the grid"""
    if not (0 <= row < grid[0] and 0 <= col < grid[1]):
        return None
    tr, tc = row // grid[2], col // grid[3]
    return tr * tiles_of(grid)[1] + tc, (row - tr * grid[2]) * grid[3] + (col - tc * grid[3])


def head_status(image, pos):
    """the update's record-head rule on the record whose content lies at pos -> (status, size)"""
    size, rtype = struct.unpack_from("<iI", image, pos - 8)
    if rtype != 2 or size < 24 or size & 7:
        return ERR_FORMAT, 0
    if size > len(image) - (pos - 8):
        return ERR_BOUNDS, 0
    return OK, size


def old_tile_reader(locate, image, decode):
    """locate(tile) -> (status, position); decode(record bytes) -> ([cells per element, an icf's as codes], [status per element])
    -> old_tile(tile): a negative status (the tile cannot be rewritten), None (no record), or the cells per element"""
    def old_tile(tile):
        st, pos = locate(tile)
        if st < 0:
            return st
        if pos == 0:
            return None
        st, size = head_status(image, pos)
        if st < 0:
            return st
        cells, status = decode(bytes(image[pos - 8:pos - 8 + size]))
        for s in status:
            if s != OK:
                return int(s)
        return cells
    return old_tile


def store(grid, elems, fills, rows, cols, values, old_tile):
    """-> (point status [n_elems, n], tiles [t] ascending, pre-status [t], {tile: cells per element after the stores})"""
    n, ne, n_cells = len(rows), len(elems), grid[2] * grid[3]
    where = [cell_of(grid, int(r), int(c)) for r, c in zip(rows, cols)]
    tiles = sorted({w[0] for w in where if w is not None})
    cells, old_status, stored = {}, {}, {t: False for t in tiles}
    for t in tiles:
        o = old_tile(t)
        old_status[t] = int(o) if isinstance(o, (int, np.integer)) else OK
        if o is None:
            cells[t] = [np.full(n_cells, BW.fill_of(el, fills[e]), BW.tile_dtype(el)) for e, el in enumerate(elems)]
        elif old_status[t] == OK:
            cells[t] = [np.array(o[e], BW.tile_dtype(el)).reshape(-1).copy() for e, el in enumerate(elems)]
    converted = [BW.set_values(np.asarray(values[e]).reshape(-1), el, fills[e]) for e, el in enumerate(elems)]
    status = np.zeros((ne, n), np.int32)
    for i in range(n):                                             # the reference's order: point after point, element after element
        if where[i] is None:
            status[:, i] = ERR_ARG
            continue
        t, at = where[i]
        if old_status[t] != OK:
            status[:, i] = old_status[t]
            continue
        for e in range(ne):
            cell, refused = converted[e]
            if refused[i]:
                status[e, i] = ERR_BOUNDS                          # setValue throws: nothing is stored, writingRequired stays
            else:
                cells[t][e][at] = cell[i]
                stored[t] = True
    pre = []
    for t in tiles:
        if old_status[t] != OK:
            pre.append(old_status[t])
        elif not stored[t]:
            pre.append(ERR_BOUNDS)
        else:
            valid = any(BW.valid_mask(cells[t][e], el, fills[e]).any() for e, el in enumerate(elems))
            pre.append(OK if valid else DECLINED)
    return status, np.array(tiles, np.int32), np.array(pre, np.int32), cells


def update(image, grid, compression, elems, fills, rows, cols, values, old_tile, encode, time_modified, force_extended=False):
    """-> (the finished image, point status, tiles, tile status, codec used [n_elems, t] with 255 for a tile without a record).
    encode(tile indices, [tiles [k, cells] per element]) -> (records, used [n_elems, k], status [k])"""
    status, tiles, pre, cells = store(grid, elems, fills, rows, cols, values, old_tile)
    if len(rows) == 0:
        return bytes(image), status, tiles, pre, np.zeros((len(elems), 0), np.uint8)
    keep = np.flatnonzero(pre == OK)
    records = [b""] * tiles.size
    used = np.full((len(elems), tiles.size), 255, np.uint8)
    tile_status = pre.copy()
    if keep.size:
        recs, u, st = encode(tiles[keep], [np.stack([cells[int(t)][e] for t in tiles[keep]]) for e in range(len(elems))])
        for k, j in enumerate(keep):
            tile_status[j] = st[k]
            if st[k] == OK:
                records[j] = recs[k]
                used[:, j] = np.asarray(u)[:, k]
    out = R.ref_update(image, tiles_of(grid)[1], compression, records, [int(t) for t in tiles], time_modified, [int(s) for s in tile_status],
                       force_extended)[0]
    return out, status, tiles, tile_status, used


# ---- standard-form records without the library: the model checked against itself on the CPU ----
def standard_decode(elems, n_cells):
    def decode(record):
        at, cells = 12, []
        for el in elems:
            (n,) = struct.unpack_from("<i", record, at)
            dt = BW.tile_dtype(el)
            cells.append(np.frombuffer(record, dt, n_cells, at + 4).copy())
            at += 4 + n
        return cells, [OK] * len(elems)
    return decode


def standard_encode(checksums):
    import gvrs_file_build as B

    def encode(idx, tiles):
        recs = [B.standard_record(int(t), [tiles[e][k] for e in range(len(tiles))], checksums) for k, t in enumerate(idx)]
        return recs, np.full((len(tiles), len(idx)), 255, np.uint8), [OK] * len(idx)
    return encode


def directory_locate(image, grid):
    """the tile directory read in place (compact or extended entries) -> locate(tile)"""
    (td,) = struct.unpack_from("<q", image, 80)
    extended = image[td + 1] != 0
    r0, c0, nr, nc = struct.unpack_from("<iiii", image, td + 8)
    n_tile_cols = tiles_of(grid)[1]

    def locate(tile):
        r, c = divmod(tile, n_tile_cols)
        if not (r0 <= r < r0 + nr and c0 <= c < c0 + nc):
            return OK, 0
        k = (r - r0) * nc + (c - c0)
        p = struct.unpack_from("<q", image, td + 24 + 8 * k)[0] if extended else struct.unpack_from("<I", image, td + 24 + 4 * k)[0] * 8
        return OK, p
    return locate
