"""A numpy model of a block write, used only by the tests: what the reference's tile cache does to the cells a user stores
(TileElementInt.java:118-126, TileElementShort.java:136-143, TileElementFloat.java:133-149, TileElementIntCodedFloat.java:152-169:
the range checks and the float-to-code conversion; TileElement*.hasValidData, RasterTile.java:215-222) on top of the cut of
tests/block_ref.py, and the layout of the records with zero-length records for the tiles RecordManager.writeTile does not write.
Elements are described as CodecMasterHip._elem_specs takes them: "int" | "short" | "float" | ("icf", scale, offset, fill_i, fill_f)."""
import numpy as np

import block_ref as B

INT_MIN, INT_MAX = -2**31, 2**31 - 1
OK, DECLINED, ERR_BOUNDS = 0, 1, -2
F32 = np.float32


def kind_of(el):
    return el if isinstance(el, str) else el[0]


def tile_dtype(el):
    """the type the record writer takes"""
    return {"int": np.int32, "short": np.int16, "icf": np.int32}.get(kind_of(el), np.float32)


def fill_of(el, fill=None):
    """the tile's fill cell: fills[e] or the default of CodecMasterHip._fill_specs; an ICF's is its code fill_i"""
    k = kind_of(el)
    if k == "icf":
        return np.int32(el[3])
    if k == "float":
        return F32(np.nan) if fill is None else F32(fill)
    return (np.int32(INT_MIN) if k == "int" else np.int16(-32768)) if fill is None else tile_dtype(el)(fill)


def default_range(el):
    """the reference's default constructors (GvrsElementSpecificationIntCodedFloat.java:113-116 in float32)"""
    k = kind_of(el)
    if k == "int":
        return INT_MIN + 1, INT_MAX
    if k == "short":
        return -32767, 32767
    if k == "float":
        return F32(-np.inf), F32(np.inf)
    scale, offset = F32(el[1]), F32(el[2])
    with np.errstate(over="ignore"):
        return F32(INT_MIN + 1) / scale + offset, F32(INT_MAX - 1) / scale + offset


def float_equals(v, fill):
    """Float.equals: the bits, every NaN being one value; +0.0 and -0.0 differ"""
    v = np.ascontiguousarray(v, F32)
    fill = F32(fill)
    same = v.view(np.uint32) == np.array([fill], F32).view(np.uint32)[0]
    return same | (np.isnan(v) & np.isnan(fill))


def icf_convert(v, el, rng=None):
    """TileElementIntCodedFloat.setValue on every cell: (codes int32, out-of-range mask; such a cell's code is fill_i)"""
    _, scale, offset, fill_i, fill_f = el
    v = np.ascontiguousarray(v, F32)
    lo, hi = default_range(el) if rng is None else (F32(rng[0]), F32(rng[1]))
    is_fill = float_equals(v, fill_f)
    with np.errstate(invalid="ignore", over="ignore"):
        in_range = (lo <= v) & (v <= hi)
        d = (v - F32(offset)) * F32(scale)                      # each rounded once in float32
        assert d.dtype == np.float32
        x = np.floor(d.astype(np.float64) + 0.5)
    code = np.where(np.isnan(x), 0.0, np.clip(x, float(INT_MIN), float(INT_MAX))).astype(np.int64)      # Java's saturating (int)
    code = np.where(is_fill | ~in_range, np.int64(fill_i), code).astype(np.int32)
    return code, ~is_fill & ~in_range


def set_values(v, el, fill=None, rng=None):
    """the block's cells of one element through setValue / setIntValue: (the tile's cells, out-of-range mask)"""
    k = kind_of(el)
    if k == "icf":
        return icf_convert(v, el, rng)
    f = fill_of(el, fill)
    lo, hi = default_range(el) if rng is None else rng
    v = np.ascontiguousarray(v, tile_dtype(el))
    if k == "float":
        with np.errstate(invalid="ignore"):
            ok = ((F32(lo) <= v) & (v <= F32(hi))) | float_equals(v, f)
    else:
        w = v.astype(np.int64)
        ok = ((w >= int(lo)) & (w <= int(hi))) | (v == f)
    return v, ~ok


def valid_mask(t, el, fill=None):
    """TileElement*.hasValidData per cell of a TILE (an ICF's cells are codes)"""
    f = fill_of(el, fill)
    if kind_of(el) == "float":
        t = np.ascontiguousarray(t, F32)
        return ~np.isnan(t) if np.isnan(f) else t != f           # the float comparison: -0.0 is the fill 0.0
    return np.asarray(t) != f


def tile_rect(grid_shape, tile_shape, rect):
    """(first tile row, first tile column, tile rows, tile columns) a rect touches (TileAccessIndices.java:79-88)"""
    r0, c0, nr, nc = rect
    tr0, tc0 = r0 // tile_shape[0], c0 // tile_shape[1]
    return tr0, tc0, (r0 + nr - 1) // tile_shape[0] - tr0 + 1, (c0 + nc - 1) // tile_shape[1] - tc0 + 1


def tile_indices(grid_shape, tile_shape, rect):
    tr0, tc0, ntr, ntc = tile_rect(grid_shape, tile_shape, rect)
    nct = B.tiles_of(grid_shape, tile_shape)[1]
    return np.array([(tr0 + i) * nct + tc0 + j for i in range(ntr) for j in range(ntc)], np.int32)


def wholly_covered(grid_shape, tile_shape, rect, idx):
    r, c = divmod(int(idx), B.tiles_of(grid_shape, tile_shape)[1])
    r0, c0, nr, nc = rect
    return r * tile_shape[0] >= r0 and c * tile_shape[1] >= c0 and (r + 1) * tile_shape[0] <= r0 + nr and (c + 1) * tile_shape[1] <= c0 + nc


def cut(grid_shape, tile_shape, rect, blocks, elems, fills=None, ranges=None, before=None):
    """(tile indices [n_out], [tiles [n_out, cells] per element in the writer's type], pre-status [n_out]).
    before: {tile index: [old cells per element] | a non-zero status (the old record cannot be read)}; entries of wholly covered
    tiles and of tiles outside the rectangle of tiles are ignored.  A tile's pre-status, first match: the old record's status,
    ERR_BOUNDS (a cell of any element out of range), DECLINED (no element has valid data), 0."""
    idx = tile_indices(grid_shape, tile_shape, rect)
    cells = tile_shape[0] * tile_shape[1]
    n = idx.size
    before = before or {}
    partial = [not wholly_covered(grid_shape, tile_shape, rect, i) for i in idx]
    pre_old = np.zeros(n, np.int32)
    for j, i in enumerate(idx):
        if partial[j] and isinstance(before.get(int(i)), (int, np.integer)):
            pre_old[j] = before[int(i)]
    bad = np.zeros(n, bool)
    valid = np.zeros(n, bool)
    tiles = []
    ones = np.ones((rect[2], rect[3]), np.int8)
    inside = B.tiles_from_block(grid_shape, tile_shape, rect, ones, idx, 0) != 0
    for e, el in enumerate(elems):
        fill = None if fills is None else fills[e]
        f = fill_of(el, fill)
        v, out = set_values(blocks[e], el, fill, None if ranges is None else ranges[e])
        old = np.full((n, cells), f, tile_dtype(el))
        for j, i in enumerate(idx):
            b = before.get(int(i))
            if partial[j] and b is not None and not isinstance(b, (int, np.integer)):
                old[j] = np.ascontiguousarray(b[e], tile_dtype(el)).reshape(-1)
        if kind_of(el) == "float":                               # cells move as bits
            t = B.tiles_from_block(grid_shape, tile_shape, rect, v.view(np.uint32), idx, 0, before=old.view(np.uint32)).view(F32)
        else:
            t = B.tiles_from_block(grid_shape, tile_shape, rect, v, idx, 0, before=old)
        tiles.append(t)
        bad |= (B.tiles_from_block(grid_shape, tile_shape, rect, out.astype(np.int8), idx, 0) != 0).any(axis=1)
        valid |= valid_mask(t, el, fill).any(axis=1)
    assert inside.any(axis=1).all()
    pre = np.where(pre_old != 0, pre_old, np.where(bad, ERR_BOUNDS, np.where(valid, OK, DECLINED))).astype(np.int32)
    return idx, tiles, pre


def expected(encode, grid_shape, tile_shape, rect, blocks, elems, fills=None, ranges=None, before=None):
    """What a block write must return: (tile indices, records with b"" for a tile without one, offsets [n_out + 1], codec used
    [n_elems, n_out] with 255 for such a tile, status [n_out]).  encode(indices, tiles per element) -> (records, used [n_elems, n],
    status [n]) is the reference-pinned record writer on the tiles whose pre-status is 0."""
    idx, tiles, pre = cut(grid_shape, tile_shape, rect, blocks, elems, fills, ranges, before)
    keep = np.flatnonzero(pre == 0)
    records = [b""] * idx.size
    used = np.full((len(elems), idx.size), 255, np.uint8)
    status = pre.copy()
    if keep.size:
        recs, u, st = encode(idx[keep], [t[keep] for t in tiles])
        for k, j in enumerate(keep):
            status[j] = st[k]
            if st[k] == 0:
                records[j] = recs[k]
                used[:, j] = u[:, k]
    offsets = np.zeros(idx.size + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in records])
    return idx, records, offsets, used, status
