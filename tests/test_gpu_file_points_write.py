"""Writes at scattered points into GVRS file images on the GPU: gf_file_update_points_elems_dev and gf_file_update_points_elems held
to the sequential model file_points_write_ref.py -- the image byte for byte, every status array item for item -- over element
mixes and codec lists, point counts that cross the waves and workgroups of the point kernels, duplicates of one cell, new tiles,
tiles that become all fill, tiles in which every value is refused, damaged old records, every edge value of
file_points_write_cases.py, points outside the grid, the allocator's order, too little room in tiles and in bytes, the round trip
through the readers, and the equivalence with the block form."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, _lib
from gridfour_amd.codec import _ptr

import block_write_ref as BW
import file_points_write_cases as K
import file_points_write_ref as M
import file_update_cases as U
import gvrs_file_build as B
import gvrs_file_update_ref as R
import gvrs_file_write_ref as W

pytestmark = pytest.mark.gpu

TILE, TILES = (5, 7), (4, 6)
GRID = (TILE[0] * TILES[0] - 1, TILE[1] * TILES[1] - 2) + TILE    # 19 x 40: the last tile row and column are cut by the grid
HELD = (0, 0, 15, 35)                                             # the base files hold records for tile rows 0..2, columns 0..4
ELEMENTS = {
    "int": B.element("z", "int", fill=-9999),
    "short": B.element("s", "short", fill=-1),
    "float": B.element("f", "float", fill=0.0),
    "icf": B.element("c", "icf", fill=-2 ** 31, scale=4.0, offset=8.0),
}
MIXES = {"mix": ("int", "short", "float", "icf"), "int": ("int",), "short": ("short",), "float": ("float",), "icf": ("icf",),
         "iss": ("int", "short", "float")}
LISTS = {"huffman": ("GvrsHuffman",), "none": (), "standard": B.STANDARD_IDS}


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


def raster(kind, seed, shape):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-500, 500, shape).astype(np.int32)
    if kind == "short":
        # few symbols: a tile's packing is shorter than its standard form; and never the fill, -1: the integer codecs carry a
        # SHORT's fill as the null code, which reads back as -32768
        return rng.integers(0, 7, shape).astype(np.int16)
    if kind == "float":
        return (rng.integers(1, 4000, shape) / 8.0).astype(np.float32)
    return (rng.integers(-4000, 4000, shape) / 4.0).astype(np.float32)     # (exact in the codes: scale 4, offset 8)


@functools.lru_cache(maxsize=None)
def base(ctx, mix, codecs, checksums=True):
    s = W.spec(GRID, [ELEMENTS[k] for k in MIXES[mix]], list(LISTS[codecs]), checksums, time_modified=5)
    rasters = [raster(k, 1 + e, HELD[2:]) for e, k in enumerate(MIXES[mix])]
    image, idx, status, _ = GvrsFileHip.write_image_host(ctx, W.lib_facts(s), rasters, rect=HELD)
    assert (status == _lib.OK).all()
    return image


class Harness:
    """a file image with what the model needs of it: the library's directory lookup, record reader and record writer"""

    def __init__(self, ctx, image):
        self.ctx, self.image = ctx, bytes(image)
        self.f = GvrsFileHip(image)
        self.grid, self.elems, self.fills = self.f.grid, self.f.elems, M.fills_of(self.f.info)
        self.master = gridfour_amd.CodecMasterHip(codec_list=self.f.info["codecs"], context=ctx)
        self.as_int = ["int" if BW.kind_of(el) == "icf" else el for el in self.elems]
        self.checksums = bool(self.f.info["checksum_enabled"])
        self.compression = len(self.f.info["codecs"]) > 0
        self.old_tile = M.old_tile_reader(self.locate, self.image, self.decode)

    def locate(self, tile):
        pos = C.c_uint64()
        st = _lib.lib().gf_file_tile_position(self.f._h, _ptr(self.f.image), self.f.image.size, int(tile), C.byref(pos))
        return st, pos.value

    def decode(self, record):
        _, cells, status = self.master.record_blob_elems(self.grid[2], self.grid[3], np.frombuffer(record, np.uint8),
                                                         np.array([0, len(record)], np.uint64), self.as_int, verify_checksums=self.checksums)
        return [c[0] for c in cells], status[:, 0].tolist()

    def encode(self, idx, tiles):
        fills = [f if BW.kind_of(el) == "short" else None for el, f in zip(self.elems, self.fills)]
        recs, used = self.master.tile_records_elems(self.grid[2], self.grid[3], idx, tiles, self.elems, self.checksums, fills)
        return recs, used, [_lib.OK] * len(recs)

    def want(self, rows, cols, values, flags=0):
        return M.update(self.image, self.grid, self.compression, self.elems, self.fills, rows, cols, values, self.old_tile, self.encode, U.TIME,
                        bool(flags & 1))


def first_negative(status):
    return next((int(s) for s in status if s < 0), _lib.OK)


def check(ctx, image, rows, cols, values, device=True, host=True, flags=0):
    """both forms against the model -> (the new image, point status, tiles, tile status)"""
    h = Harness(ctx, image)
    rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    want, w_pst, w_tiles, w_tst, w_used = h.want(rows, cols, values, flags)
    t = w_tiles.size
    u = h.f.update_begin()
    if host:
        rc, need, touched, out, pst, idx, st, used = h.f.update_points_host(ctx, u, rows, cols, values, U.TIME, flags, return_code=True)
        assert touched == t and rc == first_negative(w_tst) and need == len(want)
        assert np.array_equal(pst, w_pst) and idx.tolist() == w_tiles.tolist() and st.tolist() == w_tst.tolist()
        assert np.array_equal(used.reshape(len(h.elems), t), w_used)
        assert out == want
    if device:
        cap = h.f.update_plan_tiles(u, t)[0]
        rc, fst, n_bytes, buf, pst, idx, st, used, touched = h.f.update_points(ctx, u, rows, cols, values, U.TIME, flags, image_cap=cap, raw=True)
        assert rc == _lib.OK and fst == _lib.OK and touched == t and n_bytes == len(want)
        assert np.array_equal(pst, w_pst) and idx[:t].tolist() == w_tiles.tolist() and st[:t].tolist() == w_tst.tolist()
        assert (idx[t:] == 0x7f7f7f7f).all() and (st[t:] == 0x7f7f7f7f).all() and (used[len(h.elems) * t:] == 0x7f).all()
        assert np.array_equal(used[:len(h.elems) * t].reshape(len(h.elems), t), w_used)
        assert buf[:n_bytes] == want and set(buf[max(n_bytes, len(image)):]) <= {0xA5}, "the image differs, or a byte behind it was written"
    return want, w_pst, w_tiles, w_tst


def scatter(mix, n, seed, grid=GRID):
    """n points of the grid (duplicates as they fall) and values the elements accept"""
    rng = np.random.default_rng(seed)
    rows, cols = rng.integers(0, grid[0], n).astype(np.int32), rng.integers(0, grid[1], n).astype(np.int32)
    return rows, cols, [raster(k, seed + 10 + e, n) for e, k in enumerate(MIXES[mix])]


# ---- element mixes and codec lists ----
@pytest.mark.parametrize("mix,codecs,checksums", [("mix", "huffman", True), ("mix", "huffman", False), ("mix", "none", True), ("mix", "standard", True),
                                                 ("int", "huffman", True), ("short", "huffman", True), ("float", "huffman", True),
                                                 ("icf", "huffman", True), ("float", "standard", True)])
def test_element_mixes_and_codec_lists(ctx, mix, codecs, checksums):
    rows, cols, values = scatter(mix, 90, 3)
    _, pst, tiles, tst = check(ctx, base(ctx, mix, codecs, checksums), rows, cols, values, device=codecs != "standard")
    assert (pst == _lib.OK).all() and (tst >= _lib.OK).all() and tiles.size > 12     # (a new tile that took only its fill is declined)


def test_the_device_form_refuses_a_list_it_cannot_write(ctx):
    image = base(ctx, "mix", "standard")
    f = GvrsFileHip(image)
    rows, cols, values = scatter("mix", 5, 3)
    rc, fst, n_bytes, buf, pst, idx, st, used, touched = f.update_points(ctx, f.update_begin(), rows, cols, values, U.TIME, raw=True)
    assert rc == _lib.ERR_UNSUPPORTED and buf[:len(image)] == image and (pst == 0x7f7f7f7f).all()


# ---- point counts across the waves and workgroups of the point kernels ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_point_counts(ctx, n):
    rows, cols, values = scatter("iss", n, 100 + n)
    check(ctx, base(ctx, "iss", "huffman"), rows, cols, values)


# ---- duplicates of one cell ----
def test_duplicates_in_a_wave_a_workgroup_and_across_workgroups(ctx):
    rows, cols, values = scatter("mix", 700, 7)
    for a, b in ((3, 5), (10, 100), (20, 320), (64, 63), (255, 256), (699, 0)):     # (the later index wins wherever its lane runs)
        rows[max(a, b)], cols[max(a, b)] = rows[min(a, b)], cols[min(a, b)]
    # a later duplicate that one element refuses: the earlier value survives for that element, the later one wins for the others
    for e, (a, b) in enumerate(((40, 50), (41, 400), (42, 690), (43, 44))):
        rows[b], cols[b] = rows[a], cols[a]
        values[e][b] = [-2 ** 31, -32768, np.nan, np.inf][e]
    want, pst, tiles, tst = check(ctx, base(ctx, "mix", "huffman"), rows, cols, values)
    assert [int(pst[e, b]) for e, b in enumerate((50, 400, 690, 44))] == [_lib.ERR_BOUNDS] * 4 and (pst != 0).sum() == 4
    got, st, _ = GvrsFileHip(want).read_points_dev(ctx, rows, cols)
    last = {}
    for i in range(rows.size):
        for e in range(4):
            if pst[e, i] == 0:
                last[(e, int(rows[i]), int(cols[i]))] = values[e][i]
    assert (st == 0).all() and all(got[e][i] == last[(e, int(rows[i]), int(cols[i]))] for i in range(rows.size) for e in range(4))


# ---- tiles: new, all fill, every value refused, damaged old records ----
def tile_cells(tile, grid=GRID):
    """every cell of a tile that lies on the grid"""
    tr, tc = divmod(tile, -(-grid[1] // grid[3]))
    r, c = np.meshgrid(np.arange(tr * grid[2], min((tr + 1) * grid[2], grid[0])), np.arange(tc * grid[3], min((tc + 1) * grid[3], grid[1])),
                       indexing="ij")
    return r.ravel().astype(np.int32), c.ravel().astype(np.int32)


def join(parts):
    rows, cols = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return rows, cols, [np.concatenate([p[2][e] for p in parts]) for e in range(len(parts[0][2]))]


FILLS = {"int": -9999, "short": -1, "float": 0.0, "icf": np.nan}
REFUSED = {"int": -2 ** 31, "short": -32768, "float": np.nan, "icf": np.inf}


def constant(mix, table, n):
    return [np.full(n, table[k], BW.tile_dtype(k) if k != "icf" else np.float32) for k in MIXES[mix]]


def test_new_tiles_all_fill_tiles_and_refused_tiles(ctx):
    image = base(ctx, "mix", "huffman")
    parts = []
    for tile, n in ((20, 3), (23, 2), (5, 1)):                     # tiles without a record: in the last tile row, the grid's corner, the last column
        r, c = tile_cells(tile)
        parts.append((r[:n], c[:n], [raster(k, 30 + tile + e, n) for e, k in enumerate(MIXES["mix"])]))
    r, c = tile_cells(2)                                            # every cell becomes fill: GF_DECLINED, the record freed, the entry 0
    parts.append((r, c, constant("mix", FILLS, r.size)))
    r, c = tile_cells(3)                                            # every value is refused: the tile stays byte for byte
    parts.append((r[:9], c[:9], constant("mix", REFUSED, 9)))
    r, c = tile_cells(22)                                           # ... and a tile without a record stays without one
    parts.append((r[:2], c[:2], constant("mix", REFUSED, 2)))
    r, c = tile_cells(21)                                           # only fill stored into a new tile: GF_DECLINED, nothing to free
    parts.append((r[:2], c[:2], constant("mix", FILLS, 2)))
    rows, cols, values = join(parts)
    want, pst, tiles, tst = check(ctx, image, rows, cols, values)
    D, Bd = _lib.DECLINED, _lib.ERR_BOUNDS
    assert dict(zip(tiles.tolist(), tst.tolist())) == {2: D, 3: Bd, 5: 0, 20: 0, 21: D, 22: Bd, 23: 0}
    f, g = GvrsFileHip(image), GvrsFileHip(want)
    assert g.tile_position(2) == 0 and g.tile_position(21) == 0 and g.tile_position(22) == 0 and g.tile_position(23) != 0
    p3 = f.tile_position(3)
    (size3,) = struct.unpack_from("<i", image, p3 - 8)
    assert g.tile_position(3) == p3 and want[p3 - 8:p3 - 8 + size3] == image[p3 - 8:p3 - 8 + size3]
    # the new tiles: fill everywhere but the stored cells
    blocks, st, _ = g.read_block_dev(ctx, (15, 14, 4, 7))          # tile 20, as far as the grid reaches
    assert (st == 0).all() and blocks[0].ravel()[:3].tolist() == values[0][:3].tolist() and (blocks[0].ravel()[3:] == -9999).all()
    assert blocks[1].ravel()[:3].tolist() == values[1][:3].tolist() and (blocks[2].ravel()[3:] == 0).all() and np.isnan(blocks[3].ravel()[3:]).all()


def damaged(ctx):
    """the mix file with four hurt tiles -> (image, {tile: what was done})"""
    image = bytearray(base(ctx, "mix", "huffman"))
    f = GvrsFileHip(bytes(image))
    at, w = B.entry_offset(bytes(image), f.info, 6)
    assert w == 4
    struct.pack_into("<I", image, at, 0x7ffffff0)                  # a directory entry that leads behind the image
    p7 = f.tile_position(7)
    (size7,) = struct.unpack_from("<i", image, p7 - 8)
    struct.pack_into("<i", image, p7 - 8, size7 - 4)               # a size word that is no multiple of 8
    p8 = f.tile_position(8)
    image[p8 + 13] ^= 0x55                                          # a body whose checksum no longer holds
    p9 = f.tile_position(9)
    (n0,) = struct.unpack_from("<i", image, p9 + 4)                # element 0's bytes; element 1's packing follows its length word
    assert struct.unpack_from("<i", image, p9 + 8 + n0)[0] < 2 * TILE[0] * TILE[1]      # (a packing, not the standard form)
    image[p9 + 8 + n0 + 4] = 0x7e                                   # ... and names a codec the list does not have
    return B.refresh_record_crc(bytes(image), p9)


def test_damaged_old_records(ctx):
    image = damaged(ctx)
    parts = []
    for tile in (6, 7, 8, 9, 10):
        r, c = tile_cells(tile)
        parts.append((r[:4], c[:4], [raster(k, 50 + tile + e, 4) for e, k in enumerate(MIXES["mix"])]))
    rows, cols, values = join(parts)
    want, pst, tiles, tst = check(ctx, image, rows, cols, values)
    assert tiles.tolist() == [6, 7, 8, 9, 10]
    assert tst[0] == _lib.ERR_BOUNDS and tst[1] == _lib.ERR_FORMAT and tst[2] < 0 and tst[3] < 0 and tst[4] == 0
    for k in range(4):                                              # every element of the points takes the tile's status; nothing was stored
        assert (pst[:, 4 * k:4 * k + 4] == tst[k]).all()
    assert (pst[:, 16:] == 0).all()
    f, g = GvrsFileHip(image), GvrsFileHip(want)
    for tile in (7, 8, 9):
        p = f.tile_position(tile)
        size = struct.unpack_from("<i", base(ctx, "mix", "huffman"), p - 8)[0]
        assert g.tile_position(tile) == p and want[p - 8:p - 8 + size] == image[p - 8:p - 8 + size]
    at, _ = B.entry_offset(want, g.info, 6)
    assert struct.unpack_from("<I", want, at)[0] == 0x7ffffff0


# ---- values: every edge of the cell rule, one-element files ----
@pytest.mark.parametrize("case", range(len(K.CASES)), ids=["%s-%d" % (BW.kind_of(c[0]), k) for k, c in enumerate(K.CASES)])
def test_edge_values(ctx, case):
    el, fill, values = K.CASES[case]
    kind = BW.kind_of(el)
    if kind == "icf":
        element = B.element("c", "icf", fill=el[3], scale=el[1], offset=el[2], fill_f=el[4])
    else:
        element = B.element("v", kind, fill=fill)
    grid = (9, 14, 5, 7)
    old = raster(kind, 5, (5, 14)) if kind != "icf" else np.full((5, 14), el[2], np.float32)
    s = W.spec(grid, [element], ["GvrsHuffman"], True, time_modified=5)
    image, _, status, _ = GvrsFileHip.write_image_host(ctx, W.lib_facts(s), [old], rect=(0, 0, 5, 14))
    assert (status == _lib.OK).all()
    n = values.size
    assert n <= 28
    # each value once into a tile with a record and once into a new tile, then the refused ones again on top of stored cells
    r0, c0 = tile_cells(1, grid)
    r1, c1 = tile_cells(3, grid)
    rows, cols = np.concatenate([r0[:n], r1[:n], r0[:n]]), np.concatenate([c0[:n], c1[:n], c0[:n][::-1]])
    vals = [np.concatenate([values, values, values])]
    _, pst, tiles, tst = check(ctx, image, rows, cols, vals)
    stored, _, _ = K.expected(el, fill, values)
    assert (pst[0, :n] == np.where(stored, 0, _lib.ERR_BOUNDS)).all() and tiles.tolist() == [1, 3]


# ---- points outside the grid, mixed among valid ones ----
def test_points_outside_the_grid(ctx):
    rows, cols, values = scatter("mix", 120, 9)
    outside = [(-1, 0), (GRID[0], 0), (0, -1), (0, GRID[1]), (2 ** 31 - 1, 3), (-2 ** 31, 3), (3, 2 ** 31 - 1), (19, 39), (18, 40)]
    for k, (r, c) in enumerate(outside):
        rows[7 * k + 1], cols[7 * k + 1] = r, c
    _, pst, _, _ = check(ctx, base(ctx, "mix", "huffman"), rows, cols, values)
    assert (pst[:, [7 * k + 1 for k in range(len(outside))]] == _lib.ERR_ARG).all() and (pst == _lib.ERR_ARG).sum() == 4 * len(outside)
    # only such points: no tile is touched, and the file is closed anew
    check(ctx, base(ctx, "mix", "huffman"), [-1, GRID[0]], [0, 0], constant("mix", FILLS, 2))
    # no points at all: the image is left as it is
    image = base(ctx, "int", "huffman")
    f = GvrsFileHip(image)
    u = f.update_begin()
    out, pst, idx, st, used = f.update_points(ctx, u, [], [], [[]], U.TIME)
    assert out == image and idx.size == 0
    out, pst, idx, st, used = f.update_points_host(ctx, u, [], [], [[]], U.TIME)
    assert out == image and idx.size == 0


# ---- the allocator takes the records in ascending tile index ----
def test_allocator_order_is_ascending_tile_index(ctx):
    layout = [("t", 0, 40), ("f", 40), ("t", 1, 40), ("f", 40), ("t", 2, 40)]
    image = U.make_file(layout, compression=False)                 # 2 x 2 int cells in standard form: every new record is 40 bytes, an exact fit
    rows, cols = np.array([12, 10], np.int32), np.array([0, 0], np.int32)      # tile 60 first, then tile 50
    values = [np.array([7, 8], np.int32)]
    want, _, tiles, tst = check(ctx, image, rows, cols, values)
    assert tiles.tolist() == [50, 60] and tst.tolist() == [0, 0]
    g = GvrsFileHip(want)
    assert g.tile_position(50) < g.tile_position(60) < GvrsFileHip(image).tile_position(2)
    records = [want[p - 8:p + 32] for p in (g.tile_position(60), g.tile_position(50))]
    assert R.ref_update(image, U.N_TILE_COLS, False, records, [60, 50], U.TIME)[0] != want     # (descending order places them the other way round)


# ---- too little room ----
def test_too_little_room_in_tiles_and_in_bytes(ctx):
    image = base(ctx, "mix", "huffman")
    rows, cols, values = scatter("mix", 60, 11)
    f = GvrsFileHip(image)
    u = f.update_begin()
    t = f.cells_tiles(rows, cols).size
    rc, fst, n_bytes, buf, pst, idx, st, used, touched = f.update_points(ctx, u, rows, cols, values, U.TIME, max_tiles=t - 1, raw=True)
    assert rc == _lib.ERR_CAPACITY and touched == t
    assert buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}
    assert (pst == 0x7f7f7f7f).all() and (idx == 0x7f7f7f7f).all() and (st == 0x7f7f7f7f).all() and (used == 0x7f).all()
    assert fst == 0x7f7f7f7f and n_bytes == 0x7f7f7f7f7f7f7f7f
    rc, need, touched, out, pst, idx, st, used = f.update_points_host(ctx, u, rows, cols, values, U.TIME, max_tiles=t - 1, return_code=True)
    assert rc == _lib.ERR_CAPACITY and touched == t and out == image
    assert (pst == 0x7f7f7f7f).all() and (idx == 0x7f7f7f7f).all() and (st == 0x7f7f7f7f).all() and (used == 0x7f).all()
    want = Harness(ctx, image).want(rows, cols, values)[0]
    assert len(want) > len(image)
    rc, fst, n_bytes, buf, _, _, _, _, _ = f.update_points(ctx, u, rows, cols, values, U.TIME, image_cap=len(want) - 8, raw=True)
    assert rc == _lib.OK and fst == _lib.ERR_CAPACITY and n_bytes == len(want)
    assert buf[:len(image)] == image and set(buf[len(image):]) <= {0xA5}
    rc, need, touched, out, _, _, _, _ = f.update_points_host(ctx, u, rows, cols, values, U.TIME, image_cap=len(want) - 8, return_code=True)
    assert rc == _lib.ERR_CAPACITY and need == len(want) and out == image


# ---- the round trip ----
def test_round_trip_through_the_readers(ctx):
    image = base(ctx, "mix", "huffman")
    rows, cols, values = scatter("mix", 40, 13)
    rows, cols = (rows % 10).astype(np.int32), (cols % 21).astype(np.int32)      # tiles 0..2 and 6..8 only
    want, pst, tiles, tst = check(ctx, image, rows, cols, values)
    assert (pst == 0).all() and set(tiles.tolist()) <= {0, 1, 2, 6, 7, 8}
    f, g = GvrsFileHip(image), GvrsFileHip(want)
    report = g.inspect_dev(ctx)
    assert report.passed and report.complete
    # every cell of the touched tiles: the winning value, or the old one
    rr, cc = np.meshgrid(np.arange(10), np.arange(21), indexing="ij")
    rr, cc = rr.ravel().astype(np.int32), cc.ravel().astype(np.int32)
    old, st0, _ = f.read_points_dev(ctx, rr, cc)
    new, st1, _ = g.read_points_dev(ctx, rr, cc)
    assert (st0 == 0).all() and (st1 == 0).all()
    for e in range(4):
        expect = old[e].copy()
        for i in range(rows.size):
            expect[int(rows[i]) * 21 + int(cols[i])] = values[e][i]
        assert np.array_equal(new[e], expect)
    # records of untouched tiles keep their bytes
    for tile in range(TILES[0] * TILES[1]):
        p = f.tile_position(tile)
        if p and tile not in tiles.tolist():
            size = struct.unpack_from("<i", image, p - 8)[0]
            q = g.tile_position(tile)
            assert q == p and want[q - 8:q - 8 + size] == image[p - 8:p - 8 + size]


# ---- points that cover a tile-aligned rectangle equal the block form ----
@pytest.mark.parametrize("order", ["row-major", "shuffled"])
def test_points_over_a_rectangle_equal_the_block_form(ctx, order):
    image = base(ctx, "iss", "huffman")
    rect = (5, 7, 10, 14)                                          # tiles 7, 8, 13, 14, whole
    blocks = [raster(k, 70 + e, rect[2:]) for e, k in enumerate(MIXES["iss"])]
    blocks[0][2:7, 0:7][:] = -9999                                  # (no tile is all fill in every element: the others hold data)
    rr, cc = np.meshgrid(np.arange(rect[2]), np.arange(rect[3]), indexing="ij")
    at = np.arange(rr.size)
    if order == "shuffled":
        np.random.default_rng(5).shuffle(at)
    rows, cols = (rr.ravel()[at] + rect[0]).astype(np.int32), (cc.ravel()[at] + rect[1]).astype(np.int32)
    values = [b.ravel()[at] for b in blocks]
    f = GvrsFileHip(image)
    u = f.update_begin()
    by_block, b_idx, b_status, b_used = f.update_image(ctx, u, rect, blocks, U.TIME)
    by_points, pst, idx, st, used = f.update_points(ctx, u, rows, cols, values, U.TIME)
    assert (pst == 0).all() and idx.tolist() == b_idx.tolist() and st.tolist() == b_status.tolist() and np.array_equal(used, b_used)
    assert by_points == by_block
