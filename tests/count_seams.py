"""Helpers of the tests that run a path past a count seam (1,024 instances a round in k_codec_partition, 2^20 workgroups a grid row
in gf_tile_grid): at a million records the per-record Python of the other tests is too slow, so the framing, the CRC-32C and the
block model are written over whole arrays here.  tests/test_count_seams_inputs.py pins each of them, without a GPU, against the
per-record form it stands for (_frame / _frame_elems of tests/test_gpu_records_dev.py with the oracle's CRC-32C, tests/block_ref.py).

  frame_records / frame_records_elems   RecordManager's framing of n records whose elements have equal lengths
  assemble                              a batch drawn from a few distinct elements of any lengths: blob and offsets
  sequence                              which pool entry every record holds; none equal to the one a period before it
  block_from_tiles                      block_ref.block_from_tiles over the rectangle's tiles only, without the per-tile loop"""
import numpy as np

import block_ref

# ---- CRC-32C (Castagnoli, reflected 0x82F63B78), a byte a step over all records at once ----------------------------------------


def _crc_table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(0x82F63B78), t >> 1).astype(np.uint32)
    return t


_TABLE = _crc_table()


def crc32c_rows(rows):
    """the CRC-32C of every row of an (n, length) uint8 array: uint32 [n]"""
    rows = np.asarray(rows, np.uint8)
    crc = np.full(rows.shape[0], 0xFFFFFFFF, np.uint32)
    for col in np.ascontiguousarray(rows.T):
        crc = _TABLE[(crc ^ col) & np.uint32(0xFF)] ^ (crc >> np.uint32(8))
    return crc ^ np.uint32(0xFFFFFFFF)


# ---- framing -------------------------------------------------------------------------------------------------------------------

def _put32(records, at, values):
    records[:, at:at + 4] = np.ascontiguousarray(values, "<u4").reshape(-1, 1).view(np.uint8)


def frame_records_elems(indices, elements, crc=True):
    """n records of len(elements) elements each; elements[e] is (n, len_e) uint8.  size word, type 2, index, per element [n][bytes],
    zero padding to a multiple of 8, CRC-32C over all but the last four bytes (or 0): (n, size) uint8"""
    elements = [np.asarray(el, np.uint8) for el in elements]
    indices = np.asarray(indices)
    n = indices.size
    assert all(el.ndim == 2 and el.shape[0] == n for el in elements)
    body = sum(4 + el.shape[1] for el in elements)
    size = (4 + body + 12 + 7) // 8 * 8
    records = np.zeros((n, size), np.uint8)
    _put32(records, 0, np.full(n, size))
    records[:, 4] = 2
    _put32(records, 8, indices.astype(np.int64) & 0xFFFFFFFF)
    pos = 12
    for el in elements:
        _put32(records, pos, np.full(n, el.shape[1]))
        records[:, pos + 4:pos + 4 + el.shape[1]] = el
        pos += 4 + el.shape[1]
    if crc:
        _put32(records, size - 4, crc32c_rows(records[:, :size - 4]))
    return records


def frame_records(indices, elements, crc=True):
    """the one-element form: elements is (n, len) uint8"""
    return frame_records_elems(indices, [elements], crc)


def assemble(pool, which, indices, crc=True):
    """record t holds the elements pool[which[t]] (bytes, or a list of bytes for several elements) under tile index indices[t]; the
    records back to back: (blob uint8, offsets uint64 [n + 1]).  Records of one size are framed together."""
    which = np.asarray(which)
    indices = np.asarray(indices)
    pool = [[p] if isinstance(p, (bytes, bytearray)) else list(p) for p in pool]
    sizes = np.array([(4 + sum(4 + len(el) for el in p) + 12 + 7) // 8 * 8 for p in pool], np.int64)
    offsets = np.zeros(which.size + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes[which])
    blob = np.zeros(int(offsets[-1]), np.uint8)
    shapes = [tuple(len(el) for el in p) for p in pool]
    for shape in sorted(set(shapes[k] for k in np.unique(which))):
        ids = [k for k, s in enumerate(shapes) if s == shape]
        local = np.full(len(pool), -1)
        local[ids] = np.arange(len(ids))
        members = np.flatnonzero(local[which] >= 0)
        tables = [np.stack([np.frombuffer(bytes(pool[k][e]), np.uint8) for k in ids]).reshape(len(ids), shape[e]) for e in range(len(shape))]
        recs = frame_records_elems(indices[members], [tab[local[which[members]]] for tab in tables], crc)
        at = offsets[members].astype(np.int64)[:, None] + np.arange(recs.shape[1])[None, :]
        blob[at] = recs
    return blob, offsets


# ---- the sequence rule ---------------------------------------------------------------------------------------------------------

def sequence(seed, n, period, n_pool, placed=None):
    """Which pool entry every one of n records holds: seeded draws, the hand-placed records on top, and then no record equal to
    the one a whole number of periods before it -- a result that lands one round or one grid row off cannot go unnoticed.
    period may be a list of distances instead (records of several elements: see instance_shifts).
    (test_gpu_scratch_chunks._sequence, for any period, over whole arrays.)"""
    placed = placed or {}
    shifts = sorted(s for s in set(np.atleast_1d(period).tolist()) if 0 < s < n) if np.ndim(period) else list(range(period, n, period))
    assert n_pool > 1 + 2 * len(shifts) if np.ndim(period) else n_pool > 1 + (n - 1) // period, "more forbidden neighbours than contents"
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, n_pool, n)
    fixed = np.zeros(n, bool)
    for t, k in placed.items():
        seq[t], fixed[t] = k, True
    for _ in range(1000):
        redo = np.zeros(n, bool)
        for s in shifts:
            hit = np.flatnonzero(seq[s:] == seq[:n - s]) + s
            assert not (fixed[hit] & fixed[hit - s]).any(), "two hand-placed records a period apart are equal"
            redo[np.where(fixed[hit], hit - s, hit)] = True
        if not redo.any():
            break
        seq[redo] = rng.integers(0, n_pool, int(redo.sum()))
    for s in shifts:
        assert (seq[s:] != seq[:n - s]).all()
    for t, k in placed.items():
        assert seq[t] == k
    return seq


def instance_shifts(n_tiles, n_elems, period=1024):
    """Instances lie element-major (i = e * n_tiles + t): the distances d between two tiles such that instances of them, of any two
    elements, lie a whole number of periods apart"""
    out = set()
    for m in range(1, n_tiles * n_elems // period + 1):
        for de in range(n_elems):
            d = abs(m * period - de * n_tiles)
            if 0 < d < n_tiles:
                out.add(d)
    return sorted(out)


# ---- the block model over the rectangle's tiles --------------------------------------------------------------------------------

def block_from_tiles(grid_shape, tile_shape, rect, indices, tiles, fill, ok=None):
    """block_ref.block_from_tiles: the same cells, built over the tiles the rectangle touches only and without a Python loop over the
    list (of two entries of one tile the later one counts: numpy assigns repeated indices in order)"""
    tiles = np.asarray(tiles)
    indices = np.asarray(indices).astype(np.int64)
    tr, tc = tile_shape
    nrt, nct = block_ref.tiles_of(grid_shape, tile_shape)
    r0, c0, nr, nc = rect
    tr0, tc0, tr1, tc1 = r0 // tr, c0 // tc, (r0 + nr - 1) // tr, (c0 + nc - 1) // tc
    window = np.full((tr1 - tr0 + 1, tr, tc1 - tc0 + 1, tc), fill, tiles.dtype)
    r, c = indices // nct, indices % nct
    keep = np.flatnonzero((indices >= 0) & (indices < nrt * nct) & (r >= tr0) & (r <= tr1) & (c >= tc0) & (c <= tc1))
    cells = tiles.reshape(-1, tr, tc)[keep]
    if ok is not None:
        cells = np.where(np.asarray(ok, bool)[keep, None, None], cells, np.asarray(fill, tiles.dtype))
    window[r[keep] - tr0, :, c[keep] - tc0, :] = cells
    full = window.reshape((tr1 - tr0 + 1) * tr, (tc1 - tc0 + 1) * tc)
    return full[r0 - tr0 * tr:r0 - tr0 * tr + nr, c0 - tc0 * tc:c0 - tc0 * tc + nc].copy()


# ---- a pool of distinct tiles in every form a record can hold them --------------------------------------------------------------

POOL_SHAPE = (16, 20)                            # the shape of the partition tests; LSOP12 accepts it
POOL_SLOTS = (0, 1, 3, 4)                        # codec indices of LIST5 = (Huffman, Deflate, none, canonical, LSOP12)


def partition_pool(n=40):
    """n distinct 16 x 20 tiles, each packed once by the oracle's encoder of every integer codec of LIST5 (the packing names its
    codec index in its first byte): (tiles int32 [n, cells], {slot: [packing of tile k]}).  Every packing is shorter than the
    standard form of a SHORT element, and every cell fits a short."""
    import oracle
    from tilegen import make_tile
    r, c = POOL_SHAPE
    kinds = ["smooth", "steps", "noise8"]
    tiles = np.stack([make_tile(kinds[k % 3], r, c, seed=300 + k).astype(np.int32) + 5 * k for k in range(n)])
    assert len({t.tobytes() for t in tiles}) == n and np.abs(tiles).max() < 32767
    enc = {0: lambda v: oracle.codec_huffman_encode(0, r, c, v)[0], 1: lambda v: oracle.codec_deflate_encode(1, r, c, v)[0],
           3: lambda v: oracle.codec_canon_encode(3, r, c, v)[0], 4: lambda v: oracle.lsop12_encode(4, r, c, v, True)[0]}
    packs = {slot: [bytes(enc[slot](t)) for t in tiles] for slot in POOL_SLOTS}
    for slot, ps in packs.items():
        assert all(0 < len(p) < 2 * r * c and p[0] == slot for p in ps), slot
    return tiles, packs


def standard_form(tiles, element="int"):
    """the cells as a record holds them uncompressed (TileElementInt / TileElementShort; an even cell count: no padding)"""
    return [t.astype("<i2" if element == "short" else "<i4").tobytes() for t in tiles]
