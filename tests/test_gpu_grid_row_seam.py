"""Every later user of gf_tile_grid (gvrs_kernels.h) with more than 2^20 workgroups.  A launch of 2^20 workgroups or more is
folded into x and y; a kernel recovers its number as blockIdx.x + blockIdx.y * gridDim.x and must leave the padding of the last
grid row alone.  tests/test_gpu_full_batch.py::test_more_than_2_20_tiles* holds the codecs' kernels to that; here the record
writer (k_record_plan / k_record_scan / k_record_write / k_record_crc32c_write), the record reader's k_elem_scatter, k_block_gather,
k_block_cut_elems / k_block_write_verdict, k_grid_cut, k_downsample_direct / k_downsample_staged and the lattice kernels of
interpolation and render run with gridDim.y = 2.  Counts are SEAM + a small odd number, so the last grid row is almost all padding.
k_render_cells takes 4,096 cells per workgroup: its seam needs 2^32 cells and stays untested.

Everything is bit for bit.  Every case compares the whole output, and names the items either side of the seam (SEAM - 1, SEAM,
SEAM + 1), the first and the last one in comparisons of their own.  Contents follow count_seams.sequence with period 2^20: no
item holds what the item one grid row before it holds."""
import numpy as np
import pytest

import block_ref as B
import block_write_ref as W
import count_seams as S
import downsample_ref as DR
import records_enc_inputs as RI
from test_gpu_records_dev import ctx      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
SEAM = 1 << 20
HUFFMAN, CANON = 1, 3
CODECS = (HUFFMAN, CANON)

# ---------------------------------------------------------------- records and blocks: 1,025 x 1,025 tiles of 2 x 2 cells

TILE, TILES_ACROSS = (2, 2), 1025
GRID = (TILE[0] * TILES_ACROSS, TILE[1] * TILES_ACROSS)        # 2,050 x 2,050 cells
NT = TILES_ACROSS * TILES_ACROSS                               # 1,050,625 tiles = SEAM + 2,049
N_POOL = 32
ELEMS2 = ["int", "short"]
AT = [0, SEAM - 1, SEAM, SEAM + 1, NT - 1]


def _plan(el, cells_row):
    """(element bytes, codec used) of one tile of one element under CODECS, as CodecMaster chooses: the strictly shortest packing of
    the oracle's encoders, the list's order breaking ties, the standard form unless that is shorter"""
    best, used = None, 255
    for k, codec in enumerate(CODECS):
        pk = RI._oracle_pack(codec, k, TILE[0], TILE[1], RI.codec_cells(el, cells_row))
        if pk is not None and (best is None or len(pk) < len(best)):
            best, used = pk, k
    if best is not None and len(best) < RI.std_size(el, TILE[0] * TILE[1]):
        return bytes(best), used
    return RI.standard_form(el, cells_row), 255


class Tiles:
    """Which of 32 distinct tiles every tile of the grid holds, per element, and the records RecordManager would write for them.
    Pool entries 0 .. 15 are constant tiles (a 2 x 2 tile of one value packs to 6 bytes under the canonical codec, against 16 and 8
    in standard form), 16 .. 31 four different values each (no codec shortens those): packed and standard-form records alternate
    around the seam.  No cell is zero (what an unwritten output holds) or a fill value."""

    def __init__(self):
        rng = np.random.default_rng(2050)
        const = np.repeat(rng.permutation(np.arange(100, 3000))[:16, None], 4, axis=1)
        mixed = rng.integers(-30000, 30000, (16, 4))
        mixed[np.isin(mixed, (0, -5, -77, -99))] = 1             # (not zero, not a fill value of the tests below)
        self.cells = {"int": np.concatenate([const, 70000 * mixed]).astype(np.int32), "short": np.concatenate([-const, mixed]).astype(np.int16)}
        assert all(len({c.tobytes() for c in v}) == N_POOL for v in self.cells.values())
        placed = {0: 16, SEAM - 2: 17, SEAM - 1: 0, SEAM: 1, SEAM + 1: 18, SEAM + 2: 2, NT - 1: 3}
        self.seq = S.sequence(1025, NT, SEAM, N_POOL, placed)
        self._records = {}
        self.plans = {el: [_plan(el, row) for row in self.cells[el]] for el in ELEMS2}
        for el in ELEMS2:
            assert [u for _, u in self.plans[el]] == [1] * 16 + [255] * 16, el           # canonical | standard form

    def which(self, el):
        """the short element of a tile holds another pool entry than its int element"""
        return self.seq if el == "int" else (self.seq + 5) % N_POOL

    def values(self, el, tiles=None):
        w = self.which(el)
        return self.cells[el][w if tiles is None else w[tiles]]

    def records(self, elems, tiles=None, indices=None):
        """(blob, offsets, used [n_elems, n]) for the listed tiles (all of them) in list order"""
        key = tuple(elems) if tiles is None else None
        if key in self._records:
            return self._records[key]
        tiles = np.arange(NT) if tiles is None else np.asarray(tiles)
        if len(elems) == 1:
            pool, which = [p for p, _ in self.plans[elems[0]]], self.which(elems[0])[tiles]
        else:                                                    # (int entry k goes with short entry k + 5)
            pool = [[self.plans["int"][k][0], self.plans["short"][(k + 5) % N_POOL][0]] for k in range(N_POOL)]
            which = self.seq[tiles]
        blob, offsets = S.assemble(pool, which, tiles if indices is None else indices)
        used = np.stack([np.array([u for _, u in self.plans[el]], np.uint8)[self.which(el)[tiles]] for el in elems])
        if key:
            self._records[key] = (blob, offsets, used)               # (all tiles in order: shared by the write tests, left unchanged)
        return blob, offsets, used

    def raster(self, el):
        return self.values(el).reshape(TILES_ACROSS, TILES_ACROSS, TILE[0], TILE[1]).transpose(0, 2, 1, 3).reshape(GRID)


@pytest.fixture(scope="module")
def tiles():
    return Tiles()


@pytest.fixture(scope="module")
def master(ctx):
    import gridfour_amd
    return gridfour_amd.CodecMasterHip(codec_list=CODECS, context=ctx)


def _same_records(got_blob, got_off, want_blob, want_off, what):
    assert np.array_equal(got_off, want_off), (what, "offsets", np.flatnonzero(got_off != want_off)[:4])
    o = want_off.astype(np.int64)
    for t in AT:
        assert got_blob[o[t]:o[t + 1]].tobytes() == want_blob[o[t]:o[t + 1]].tobytes(), (what, "record", t)
    total = int(o[-1])
    if not np.array_equal(got_blob[:total], want_blob):
        at = int(np.flatnonzero(got_blob[:total] != want_blob)[0])
        raise AssertionError((what, "first differing byte", at, "in record", int(np.searchsorted(o, at, "right")) - 1))


@pytest.mark.parametrize("elems", [["int"], ELEMS2], ids=["int", "int+short"])
def test_more_than_2_20_records_written(master, tiles, elems):
    """gf_tile_record_encode_batch_elems_dev on all 1,050,625 tiles of 2 x 2 cells (a 4-cell tile does pack: see Tiles): k_record_plan,
    k_record_scan over 1,026 blocks of 1,024, k_record_write on nTiles * nElems workgroups (with two elements the seam falls
    inside element 0 and element 1 lies wholly in the second grid row), k_record_crc32c_write.  The whole blob, every offset and
    every codec-used byte against the vectorised framing of tests/count_seams.py."""
    want_blob, want_off, want_used = tiles.records(elems)
    blob, offsets, used, status = master.tile_records_elems_dev(TILE[0], TILE[1], np.arange(NT), [tiles.values(el) for el in elems], elems, raw=True)
    assert (status == 0).all(), np.flatnonzero(status)[:8]
    assert np.array_equal(used, want_used), np.argwhere(used != want_used)[:8]
    assert (used[:, SEAM - 1:SEAM + 1] == 1).all() and (used[:, SEAM + 1] == 255).all()      # packed and standard form at the seam
    _same_records(blob, offsets, want_blob, want_off, elems)


def _shuffled(tiles):
    """the records of all tiles but five in shuffled order, one tile twice (with other cells in its first record): the list of
    tiles record by record, and for the duplicate's first record the tile whose cells it holds"""
    rng = np.random.default_rng(77)
    absent = np.array([0, 1024, SEAM, NT - 1, 555555])
    order = rng.permutation(np.setdiff1d(np.arange(NT), absent))
    twice, other = int(order[SEAM + 1]), int(order[7])
    content = order.copy()
    order = np.insert(order, 3, twice)                           # record 3: tile `twice` with the cells of tile `other`; the later one counts
    content = np.insert(content, 3, other)
    assert order.size == NT - 4 and order.size > SEAM + 1
    return absent, order, content


@pytest.mark.parametrize("rect", [(0, 0) + GRID, (1, 1, 2048, 2048)], ids=["whole", "inset"])
def test_more_than_2_20_tiles_read_as_a_block(master, tiles, rect):
    """gf_block_read_elems_dev over records of INT + SHORT tiles: 2 x 1,050,621 element instances through the partition's 2,052
    rounds and k_elem_scatter, then k_block_gather on nElems * 1,025 * 1,025 workgroups -- the seam falls inside element 0, and
    w = e * nRect + k carries element 1 across it.  The inset rectangle still touches every tile.  Every cell against the model
    (count_seams.block_from_tiles, pinned to block_ref.block_from_tiles by tests/test_count_seams_inputs.py; block_ref itself on
    the tiles at the seam)."""
    absent, order, content = _shuffled(tiles)
    blob, offsets, _ = tiles.records(ELEMS2, tiles=content, indices=order)
    fills = [-77, -99]
    blocks, st = master.read_block_dev(TILE[0], TILE[1], GRID, rect, blob, offsets, ELEMS2, fills=fills)
    assert st.shape == (2, order.size) and (st == 0).all(), np.argwhere(st)[:8]
    r0, c0, nr, nc = rect
    for e, el in enumerate(ELEMS2):
        cells = tiles.values(el, content)
        want = S.block_from_tiles(GRID, TILE, rect, order, cells, fills[e])
        assert (want == fills[e]).sum() == sum(1 if rect[0] and t in (0, 1024, NT - 1) else 4 for t in absent)
        # the tiles of the gather's workgroups 0, SEAM - 1, SEAM, SEAM + 1 and the last one: tile k of the grid, for both elements
        for k in AT:
            ty, tx = divmod(k, TILES_ACROSS)
            ra, rb, ca, cb = max(2 * ty, r0), min(2 * ty + 2, r0 + nr), max(2 * tx, c0), min(2 * tx + 2, c0 + nc)
            j = np.flatnonzero(order == k)
            ref = B.block_from_tiles(GRID, TILE, (ra, ca, rb - ra, cb - ca), order[j], cells[j], fills[e])
            assert np.array_equal(blocks[e][ra - r0:rb - r0, ca - c0:cb - c0], ref), (el, "tile", k)
        wrong = np.argwhere(blocks[e] != want)
        assert wrong.size == 0, (el, rect, len(wrong), wrong[:4], "tiles", [(int(r + r0) // 2) * TILES_ACROSS + int(c + c0) // 2 for r, c in wrong[:4]])


def test_more_than_2_20_tiles_written_from_a_block(master, tiles):
    """gf_block_write_elems_dev of the whole 2,050 x 2,050 grid, INT + SHORT: k_block_cut_elems and k_block_write_verdict on 1,050,625
    tiles, then the record writer.  The model of the cut and the verdicts (tests/block_write_ref.py) is evaluated on the first row
    of tiles, the row that holds tiles SEAM - 1, SEAM and SEAM + 1, and the last; the whole blob, offsets, indices, codec-used and
    statuses against the framing of the tiles the raster was built from."""
    rasters = [tiles.raster(el) for el in ELEMS2]
    want_blob, want_off, want_used = tiles.records(ELEMS2)
    for ty in (0, SEAM // TILES_ACROSS, TILES_ACROSS - 1):       # the model: one row of tiles at a time
        rect = (2 * ty, 0, 2, GRID[1])
        idx, cut, pre = W.cut(GRID, TILE, rect, [r[2 * ty:2 * ty + 2] for r in rasters], ELEMS2)
        assert np.array_equal(idx, np.arange(ty * TILES_ACROSS, (ty + 1) * TILES_ACROSS)) and (pre == 0).all()
        for e, el in enumerate(ELEMS2):
            assert np.array_equal(cut[e], tiles.values(el, idx)), (el, ty)
    assert SEAM // TILES_ACROSS * TILES_ACROSS == SEAM - 1
    idx, blob, offsets, used, status = master.write_block_dev(TILE[0], TILE[1], GRID, (0, 0) + GRID, rasters, ELEMS2, raw=True)
    assert np.array_equal(idx, np.arange(NT)), np.flatnonzero(idx != np.arange(NT))[:8]
    assert (status == 0).all(), (np.flatnonzero(status)[:8], status[status != 0][:8])
    assert np.array_equal(used, want_used), np.argwhere(used != want_used)[:8]
    _same_records(blob, offsets, want_blob, want_off, "block write")


def test_more_than_2_20_tiles_cut_from_a_grid(ctx, tiles):
    """gf_tiles_from_block_dev (k_grid_cut) on a list of SEAM + 5 tiles of that grid in shuffled order, two indices outside the
    grid among them, from the inset rectangle: the edge tiles are part fill.  Every tile against the raster cut by a reshape, and
    block_ref.tiles_from_block on the list's entries at the seam."""
    import gridfour_amd
    n = SEAM + 5
    rng = np.random.default_rng(5)
    listed = rng.permutation(NT)[:n].astype(np.int32)
    listed[[9, SEAM + 2]] = [NT, -1]
    listed[[0, SEAM - 1, SEAM, SEAM + 1, n - 1]] = [1024, NT - 1, 0, 1025 * 1024, 515]       # the grid's corners where the seam is
    rect, fill = (1, 1, 2048, 2048), -5
    raster = tiles.raster("int")
    block = np.ascontiguousarray(raster[1:2049, 1:2049])
    full = np.full(GRID, fill, np.int32)
    full[1:2049, 1:2049] = block
    cut_all = full.reshape(TILES_ACROSS, 2, TILES_ACROSS, 2).transpose(0, 2, 1, 3).reshape(NT, 4)
    good = (listed >= 0) & (listed < NT)
    d_block = gridfour_amd.DeviceBuffer(ctx, block.nbytes + 16).upload(block)
    d_idx = gridfour_amd.DeviceBuffer(ctx, n * 4 + 16).upload(listed)
    d_tiles = gridfour_amd.DeviceBuffer(ctx, (n + 16) * 16).fill(0x5A)
    d_st = gridfour_amd.DeviceBuffer(ctx, n * 4 + 16).fill(0x5A)
    try:
        ctx.tiles_from_block_dev(GRID + TILE, rect, 0, fill, d_block.ptr, n, d_idx.ptr, d_tiles.ptr, d_st.ptr)
        ctx.synchronize()
        got = d_tiles.download(np.int32, (n + 16) * 4).reshape(n + 16, 4)
        st = d_st.download(np.int32, n)
    finally:
        for b in (d_block, d_idx, d_tiles, d_st):
            b.free()
    assert np.array_equal(st, np.where(good, 0, -2)), np.flatnonzero(st != np.where(good, 0, -2))[:8]
    assert (got[n:] == 0x5A5A5A5A).all() and (got[:n][~good] == 0x5A5A5A5A).all()              # nothing behind the list, nothing for a bad index
    at = [0, SEAM - 1, SEAM, SEAM + 1, n - 1]
    assert np.array_equal(got[at], B.tiles_from_block(GRID, TILE, rect, block, listed[at], fill)), "the entries at the seam"
    wrong = np.flatnonzero((got[:n][good] != cut_all[listed[good]]).any(axis=1))
    assert wrong.size == 0, (wrong.size, np.flatnonzero(good)[wrong[:8]])


# ---------------------------------------------------------------- downsample: SEAM + 3 output rows

DS_CASES = [(1, DR.SHORT, 3, 0), (1, DR.FLOAT, 1, 0),
            (2, DR.INT, 3, 0),                   # col0 = 0, a pitch of 6 cells: the 8-byte load of a window row applies
            (2, DR.INT, 3, 1),                   # col0 = 1, a pitch of 7: it does not
            (3, DR.INT, 1, 0),
            (9, DR.SHORT, 1, 0)]                 # k_downsample_staged; the block is 85 M cells


def _ds_block(rng, shape, elem_type, fill):
    """random cells over the type's range in the lower half of the block and small ones in the upper, the fill value sprinkled so
    that about one window in five holds one; floats with NaN and -0.0 among them"""
    n = shape[0] * shape[1]
    if elem_type == DR.FLOAT:
        v = rng.uniform(-1000.0, 1000.0, shape).astype(np.float32)
        v.reshape(-1)[rng.integers(0, n, n // 50)] = np.nan
        v.reshape(-1)[rng.integers(0, n, n // 50)] = -0.0
        return v
    dt = DR.DTYPES[elem_type]
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    v[:shape[0] // 2] = rng.integers(-40, 41, (shape[0] // 2, shape[1]), dtype=dt)
    return v


@pytest.mark.parametrize("f,elem_type,c,col0", DS_CASES, ids=["f%d-%s-c%d-col%d" % (f, "isf"[t], c, o) for f, t, c, o in DS_CASES])
def test_more_than_2_20_downsample_workgroups(ctx, f, elem_type, c, col0):
    """a block of f * (SEAM + 3) rows and f * c (+ col0) columns: SEAM + 3 output rows of c cells, one workgroup each (dsPlace, wg0,
    the padding guard at.i >= outRows).  The whole output against tests/downsample_ref.py."""
    from test_gpu_downsample import run_dev
    n_out = SEAM + 3
    block = (0, col0, f * n_out, f * c + col0)
    fill = {DR.INT: -2 ** 31, DR.SHORT: -32768, DR.FLOAT: 0}[elem_type]
    rng = np.random.default_rng(100 * f + elem_type + col0)
    v = _ds_block(rng, block[2:], elem_type, fill)
    if elem_type != DR.FLOAT:
        sprinkle = rng.integers(0, v.size, n_out * c // 5)
        v.reshape(-1)[sprinkle] = fill
    assert DR.out_rect(block, f) == (0, -(-col0 // f), n_out, c)
    got = run_dev(ctx, [(elem_type, fill, v)], block, f)[0]
    want = DR.downsample(v, block, f, elem_type, fill)
    for i in (0, SEAM - 1, SEAM, SEAM + 1, n_out - 1):
        assert DR.same_bits(got[i], want[i]), (f, elem_type, "output row", i, got[i], want[i])
    if elem_type == DR.FLOAT:
        assert np.isnan(want).any() and not np.isnan(want[SEAM - 1:SEAM + 2]).all()
    else:
        assert (want == fill).any() and (want[SEAM - 1:SEAM + 2] != fill).any()
    assert DR.same_bits(got, want), np.argwhere(got.view(np.uint8).reshape(want.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,)))[:4]


# ---------------------------------------------------------------- interpolation and render: lattices of SEAM + 1 patches

LAT_ROWS = 16 * SEAM + 5                         # patches of 16 rows x 64 columns: SEAM + 1 of them, the last one of 5 rows
LAT_CASES = [(0, 0), (1, 1)]                     # (wrap, target): VALUE without wrap, FIRST with wrapped columns
LAT_SLICES = [(0, 16), (16 * (SEAM - 1), LAT_ROWS)]      # the first patch; patches SEAM - 1 and SEAM (the last, partial one)
OUT_BAND = 256


def _tall_lattice(wrap):
    """one column of 16 * SEAM + 5 points whose rows sweep the 12 x 14 grid from inside one fringe (-0.45) to inside the other (11.45):
    the patches at the seam lie at the lattice's end, and every point there has a value; with wrap 1 the column's window wraps"""
    return (-0.45, 5.3 if wrap == 0 else -0.3, 11.9 / LAT_ROWS, 0.0, LAT_ROWS, 1)


def _part(d, a, b):
    return {k: v[a:b] for k, v in d.items()}


@pytest.mark.parametrize("wrap,target", LAT_CASES, ids=["value", "first-wrap"])
def test_more_than_2_20_interp_patches(ctx, wrap, target):
    """k_interp_lattice with patchCols = 1, patchRows = SEAM + 1 (the padding guard i0 >= latRows): z and status of all 16.8 M points
    equal the points form on the same coordinates (k_interp_points, a 1-D grid at this size); the numpy model on the first patch
    and on patches SEAM - 1 and SEAM, the last."""
    import interp_cases as K
    import interp_ref as R
    import test_gpu_interp as TI
    rng = np.random.default_rng(4000 + wrap)
    spec = R.Spec(12, 14, None, R.FLOAT, wrap=wrap, target=target, row_spacing=0.9, col_spacing=1.1)
    block = K.random_block(rng, R.FLOAT, (12, 14))
    lattice = _tall_lattice(wrap)
    rows, cols = R.lattice_coords(*lattice)
    got = TI.run_lattice(ctx, spec, block, lattice, outs=["z", "status"])
    for a, b in LAT_SLICES:
        want = R.interp(spec, block, rows[a:b], cols[a:b])
        assert (want["status"] == R.OK).all() and not np.isnan(want["z"]).any()
        K.assert_same(_part(got, a, b), {k: want[k] for k in got}, ("model", a, b))
    assert (got["status"] == R.OK).all()
    K.assert_same(TI.run_points(ctx, spec, block, rows, cols, outs=["z", "status"]), got, "points form")


@pytest.mark.parametrize("wrap,target", LAT_CASES, ids=["value", "first-wrap"])
def test_more_than_2_20_render_patches(ctx, wrap, target):
    """k_render_lattice the same way: argb and status against the points form of the render (k_render_points) and the model of
    tests/render_ref.py; a light, and so first derivatives, in the second case"""
    import gridfour_amd
    import interp_cases as K
    import interp_ref as R
    import render_cases as RC
    import render_ref as M
    import test_gpu_interp as TI
    import test_gpu_render as TR
    rng = np.random.default_rng(4100 + wrap)
    args = dict(records=RC._ramp(9, -70.0, 70.0, gaps=True), argb_for_null=0xff00ff00)
    model, pal = M.Palette(**args), gridfour_amd.Palette(ctx, **args)
    light = RC.LIGHTS["cog"] if target else None
    spec = R.Spec(12, 14, None, R.FLOAT, wrap=wrap, row_spacing=0.9, col_spacing=1.1)
    block = K.random_block(rng, R.FLOAT, (12, 14))
    lattice = _tall_lattice(wrap)
    rows, cols = R.lattice_coords(*lattice)
    s, li, outs = K.lib_spec(spec), RC.lib_light(light), ("argb", "status")
    got = TR._run_render(ctx, spec, block, LAT_ROWS, lambda d_block, o: ctx.render_lattice_dev(s, d_block, lattice, pal, o, li), outs)
    for a, b in LAT_SLICES:
        want = M.render_points(spec, block, rows[a:b], cols[a:b], model, light)
        TR._assert_render(_part(got, a, b), want, ("model", a, b))
    assert len(set(got["argb"][::4099].tolist())) > 50 and (got["status"] == R.OK).all()
    d_rows, d_cols = TI._up(ctx, rows), TI._up(ctx, cols)
    try:
        by_points = TR._run_render(ctx, spec, block, LAT_ROWS, lambda d_block, o: ctx.render_points_dev(s, d_block, pal, o, n_points=LAT_ROWS, d_rows=d_rows.ptr,
                                                                                                      d_cols=d_cols.ptr, light=li), outs)
    finally:
        d_rows.free()
        d_cols.free()
        pal.close()
    TR._assert_render(by_points, got, "points form")


# ---------------------------------------------------------------- interpolation and render: the points kernels, 2^28 points

PT_ROWS, PT_COLS = SEAM + 3, 256                 # a lattice with a column spacing per row goes to k_*_points, 256 points a workgroup
PT_LATTICE = (-0.45, -0.8, 11.9 / PT_ROWS, 15.5 / PT_COLS, PT_ROWS, PT_COLS)         # rows as _tall_lattice; columns beyond both fringes
PT_ROW_SLICES = [(0, 2), (SEAM - 1, SEAM + 2), (PT_ROWS - 2, PT_ROWS)]
PIECE = 1 << 25                                  # items of a download: 256 MB of doubles


def _pt_coords(a, b):
    r = np.float64(PT_LATTICE[0]) + np.arange(a, b, dtype=np.float64) * np.float64(PT_LATTICE[2])
    c = np.float64(PT_LATTICE[1]) + np.arange(PT_COLS, dtype=np.float64) * np.float64(PT_LATTICE[3])
    return np.repeat(r, PT_COLS), np.tile(c, b - a)


def _same_in_pieces(d_a, d_b, dtype, n, what):
    """two device arrays of n items between guard bands of OUT_BAND bytes, downloaded and compared in pieces (a NaN's bits too: both
    kernels write the same NaN)"""
    for b in (d_a, d_b):
        assert (b.download(np.uint8, OUT_BAND) == 0xA5).all() and (b.download(np.uint8, OUT_BAND, OUT_BAND + n * np.dtype(dtype).itemsize) == 0xA5).all(), what
    for at in range(0, n, PIECE):
        m = min(PIECE, n - at)
        x = d_a.download(dtype, m, OUT_BAND + at * np.dtype(dtype).itemsize)
        y = d_b.download(dtype, m, OUT_BAND + at * np.dtype(dtype).itemsize)
        assert np.array_equal(x, y), (what, "first differing item", at + int(np.flatnonzero(x != y)[0]))


def _guarded(ctx, nbytes):
    """nbytes of output between guard bands; only the bands are pre-set (the kernels write every item)"""
    import gridfour_amd
    b = gridfour_amd.DeviceBuffer(ctx, nbytes + 2 * OUT_BAND)
    band = np.full(OUT_BAND, 0xA5, np.uint8)
    b.upload(band)
    b.upload(band, OUT_BAND + nbytes)
    return b


def test_more_than_2_20_interp_point_workgroups(ctx):
    """k_interp_points on SEAM + 3 workgroups: a lattice of SEAM + 3 rows x 256 columns with a column spacing per row, z alone
    (2.1 GB).  All 2^28 + 768 values equal the lattice kernel's with that one spacing, bit for bit; the model on the rows at the
    seam and at both ends.  4.3 GB of device memory, downloads of 256 MB; 0.6 s on an MI355X."""
    import gridfour_amd
    import interp_cases as K
    import interp_ref as R
    rng = np.random.default_rng(4200)
    spec = R.Spec(12, 14, None, R.FLOAT, wrap=1, target=R.FIRST, row_spacing=0.9, col_spacing=0.75)
    block = K.random_block(rng, R.FLOAT, (12, 14))
    n = PT_ROWS * PT_COLS
    s = K.lib_spec(spec)
    d_block = gridfour_amd.DeviceBuffer(ctx, block.nbytes + 16).upload(block)
    d_cs = gridfour_amd.DeviceBuffer(ctx, PT_ROWS * 8 + 16).upload(np.full(PT_ROWS, 0.75))
    d_pts, d_lat = _guarded(ctx, n * 8), _guarded(ctx, n * 8)
    try:
        ctx.interp_lattice_dev(s, d_block.ptr, PT_LATTICE, {"z": d_pts.ptr.value + OUT_BAND}, d_cs.ptr)
        ctx.interp_lattice_dev(s, d_block.ptr, PT_LATTICE, {"z": d_lat.ptr.value + OUT_BAND})
        ctx.synchronize()
        for a, b in PT_ROW_SLICES:
            rows, cols = _pt_coords(a, b)
            want = R.interp(spec, block, rows, cols)["z"]
            got = d_pts.download(np.float64, (b - a) * PT_COLS, OUT_BAND + a * PT_COLS * 8)
            assert R.same_bits(got, want) and not np.isnan(want).all(), ("model, rows", a, b)
        _same_in_pieces(d_pts, d_lat, np.uint64, n, "points kernel | lattice kernel")
    finally:
        for b in (d_block, d_cs, d_pts, d_lat):
            b.free()


def test_more_than_2_20_render_point_workgroups(ctx):
    """k_render_points the same way, argb alone (1.1 GB), with a light; 0.4 s on an MI355X"""
    import gridfour_amd
    import interp_cases as K
    import interp_ref as R
    import render_cases as RC
    import render_ref as M
    rng = np.random.default_rng(4300)
    args = dict(records=RC._ramp(9, -70.0, 70.0, gaps=True), argb_for_null=0xff00ff00)
    model, pal = M.Palette(**args), gridfour_amd.Palette(ctx, **args)
    light = RC.LIGHTS["extract"]
    spec = R.Spec(12, 14, None, R.FLOAT, wrap=1, row_spacing=0.9, col_spacing=0.75)
    block = K.random_block(rng, R.FLOAT, (12, 14))
    n = PT_ROWS * PT_COLS
    s, li = K.lib_spec(spec), RC.lib_light(light)
    d_block = gridfour_amd.DeviceBuffer(ctx, block.nbytes + 16).upload(block)
    d_cs = gridfour_amd.DeviceBuffer(ctx, PT_ROWS * 8 + 16).upload(np.full(PT_ROWS, 0.75))
    d_pts, d_lat = _guarded(ctx, n * 4), _guarded(ctx, n * 4)
    try:
        ctx.render_points_dev(s, d_block.ptr, pal, {"argb": d_pts.ptr.value + OUT_BAND}, lattice=PT_LATTICE, d_col_spacing=d_cs.ptr, light=li)
        ctx.render_lattice_dev(s, d_block.ptr, PT_LATTICE, pal, {"argb": d_lat.ptr.value + OUT_BAND}, li)
        ctx.synchronize()
        for a, b in PT_ROW_SLICES:
            rows, cols = _pt_coords(a, b)
            want = M.render_points(spec, block, rows, cols, model, light)["argb"]
            got = d_pts.download(np.uint32, (b - a) * PT_COLS, OUT_BAND + a * PT_COLS * 4)
            assert np.array_equal(got, want) and (want != model.argb_for_null).any(), ("model, rows", a, b)
        _same_in_pieces(d_pts, d_lat, np.uint32, n, "points kernel | lattice kernel")
    finally:
        for b in (d_block, d_cs, d_pts, d_lat):
            b.free()
        pal.close()
