"""Rectangles at the far corner of a real-sized grid.  The block, interpolation and render tests work on grids of 9 x 11 to some
100 x 100 cells, and the argument tests probe 2^31 - 1 without a device; here the kernels run on the GEBCO shape of BASELINE.json
-- 43,200 x 86,400 cells in 200 x 200 tiles, 93,312 tiles -- at its last rows and columns, and once on the largest grids the
argument checks accept (tests/test_blocks_args.py: 0x7fffffff tiles; tests/test_interp_args.py: 2^31 - 1 rows and columns), so that
the tile arithmetic, the 64-bit addresses and the int / double window rules see coordinates of five and ten digits.

The numpy models of tests/block_ref.py and tests/block_write_ref.py lay out the whole grid (15 GB at this shape), so they are
evaluated on the 2 x 2 tiles a rectangle touches as a grid of their own and the tile indices are translated by whole tiles: both
models depend on a rectangle only through its place relative to the tile boundaries.  tests/downsample_ref.py, interp_ref.py and
render_ref.py take the real coordinates.  Records exist only for the tiles that are touched; everything is bit for bit."""
import numpy as np
import pytest

import block_ref as B
import block_write_ref as W
import downsample_ref as DR
import interp_cases as K
import interp_ref as R
import render_cases as RC
import render_ref as M
import test_gpu_interp as TI
import test_gpu_render as TR
from test_gpu_block_write import crop, rasters
from test_gpu_records_dev import _concat
from test_gpu_records_dev import ctx      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
HUFFMAN, CANON = 1, 3
F32 = np.float32
ELEMS = ["int", "short", "float"]
FILLS = [-123456, -32768, F32(-7.5)]           # (values the smooth rasters do not hold; SHORT: the one fill a packed tile's fill cells read back as)
TYPES = [DR.INT, DR.SHORT, DR.FLOAT]


class Corner:
    """shape = (tile rows, tile columns) tiles of a large grid as a small grid of their own: first = (tile row, tile column) of the
    upper left one"""

    def __init__(self, grid, tile, first, shape=(2, 2)):
        self.grid, self.tile, self.first, self.shape = grid, tile, first, shape
        self.small = (shape[0] * tile[0], shape[1] * tile[1])
        self.across = B.tiles_of(grid, tile)[1]
        assert first[0] + shape[0] <= B.tiles_of(grid, tile)[0] and first[1] + shape[1] <= self.across

    def index(self, small_idx):
        """tile indices of the small grid -> of the large one"""
        ty, tx = np.divmod(np.asarray(small_idx, np.int64), self.shape[1])
        return ((ty + self.first[0]) * self.across + tx + self.first[1]).astype(np.int32)

    def rect(self, small_rect):
        return (small_rect[0] + self.first[0] * self.tile[0], small_rect[1] + self.first[1] * self.tile[1]) + tuple(small_rect[2:])


GEBCO, TILE = (43200, 86400), (200, 200)
CORNERS = {"the last four tiles": Corner(GEBCO, TILE, (214, 430)), "the middle of the last tile row": Corner(GEBCO, TILE, (214, 215))}
SMALL_RECT = (196, 195, 9, 11)                   # rows 196 .. 204, columns 195 .. 205 of the 400 x 400 corner: across all four tiles


@pytest.fixture(scope="module")
def master(ctx):
    import gridfour_amd
    return gridfour_amd.CodecMasterHip(codec_list=(HUFFMAN, CANON), context=ctx)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _tiles_of(corner, seed):
    """the four tiles of the corner cut from smooth rasters: [cells [4, 40000] per element]"""
    idx, tiles, pre = W.cut(corner.small, corner.tile, (0, 0) + corner.small, rasters(ELEMS, corner.small, seed), ELEMS, FILLS)
    assert list(idx) == [0, 1, 2, 3] and (pre == 0).all()
    return tiles


def _records(master, corner, tiles, listed):
    """the records of the listed tiles of the corner, under their indices on the large grid"""
    recs, used = master.tile_records_elems(corner.tile[0], corner.tile[1], corner.index(listed), [t[listed] for t in tiles], ELEMS, fills=FILLS)
    assert (used != 255).any()                                   # the codecs win on the smooth rasters: packed elements among them
    return recs


@pytest.mark.parametrize("where", list(CORNERS))
def test_blocks_read_at_the_far_corner(master, where):
    """gf_block_read_elems_dev and gf_block_read_downsampled_elems_dev (f = 3) on a 9 x 11 rectangle across four tiles of the GEBCO
    grid; the tile in the lower left has no record and reads as fill"""
    corner = CORNERS[where]
    rect = corner.rect(SMALL_RECT)
    assert rect[0] + 9 > 43000 > rect[0] and rect[1] % 200 == 195 and rect[0] + rect[2] <= GEBCO[0] and rect[1] + rect[3] <= GEBCO[1]
    tiles = _tiles_of(corner, seed=3)
    listed = np.array([3, 0, 1])
    blob, offsets = _concat(_records(master, corner, tiles, listed))
    blocks, st = master.read_block_dev(TILE[0], TILE[1], GEBCO, rect, blob, offsets, ELEMS, fills=FILLS)
    coarse, cst = master.read_block_downsampled_dev(TILE[0], TILE[1], GEBCO, rect, 3, blob, offsets, ELEMS, fills=FILLS)
    assert (st == 0).all() and (cst == 0).all()
    out = DR.out_rect(rect, 3)
    assert out[2:] == (3, 3)
    for e, el in enumerate(ELEMS):
        fill = np.asarray(FILLS[e], tiles[e].dtype).reshape(1)
        want = B.block_from_tiles(corner.small, TILE, SMALL_RECT, listed, _bits(tiles[e][listed]), _bits(fill)[0]).view(tiles[e].dtype)
        assert (want[5:, :5] == fill[0]).all() and (want[:4] != fill[0]).all()                 # the absent tile's share, and no other cell
        assert np.array_equal(_bits(blocks[e]), _bits(want)), (where, el)
        assert DR.same_bits(coarse[e], DR.downsample(want, rect, 3, TYPES[e], FILLS[e])), (where, el, "f = 3")


@pytest.mark.parametrize("where", list(CORNERS))
def test_blocks_written_at_the_far_corner(master, where):
    """gf_block_write_elems_dev of the same rectangles over old records (read-modify-write: all four tiles are partly covered; the
    file holds three of them) against tests/block_write_ref.py"""
    corner = CORNERS[where]
    rect = corner.rect(SMALL_RECT)
    old_tiles = _tiles_of(corner, seed=5)
    held = np.array([2, 0, 3])
    old = _concat(_records(master, corner, old_tiles, held))
    before = {int(t): [old_tiles[e][t] for e in range(len(ELEMS))] for t in held}
    blocks = crop(rasters(ELEMS, corner.small, seed=9), SMALL_RECT)

    def encode(indices, tiles):
        return master.tile_records_elems_dev(TILE[0], TILE[1], corner.index(indices), tiles, ELEMS, fills=FILLS)
    w_idx, w_recs, _, w_used, w_st = W.expected(encode, corner.small, TILE, SMALL_RECT, blocks, ELEMS, FILLS, None, before)
    idx, recs, used, st = master.write_block_dev(TILE[0], TILE[1], GEBCO, rect, blocks, ELEMS, fills=FILLS, old=old)
    assert np.array_equal(idx, corner.index(w_idx)) and idx.max() == (93311 if "four" in where else 93311 - 215), idx
    assert np.array_equal(st, w_st) and (st == 0).all() and np.array_equal(used, w_used)
    assert recs == w_recs, [j for j in range(4) if recs[j] != w_recs[j]]
    # the file read back with the new records behind the old ones: the old cells around the rectangle, the new ones inside
    blob, offsets = _concat([bytes(old[0][int(a):int(b)]) for a, b in zip(old[1][:-1], old[1][1:])] + recs)
    around = corner.rect((190, 190, 20, 20))
    back, bst = master.read_block_dev(TILE[0], TILE[1], GEBCO, around, blob, offsets, ELEMS, fills=FILLS)
    assert (bst == 0).all()
    for e in range(len(ELEMS)):
        fill = np.asarray(FILLS[e], old_tiles[e].dtype).reshape(1)
        want = B.block_from_tiles(corner.small, TILE, (190, 190, 20, 20), held, _bits(old_tiles[e][held]), _bits(fill)[0]).view(old_tiles[e].dtype)
        want[6:15, 5:16] = blocks[e]
        assert np.array_equal(_bits(back[e]), _bits(want)), (where, e)


def test_blocks_on_the_largest_grid_the_checks_accept(ctx):
    """0x7fffffff tiles, the bound of tests/test_blocks_args.py::test_limits_are_unsupported (a Mersenne prime: one row or one column
    of tiles): a grid of 2^31 - 1 rows x 11 columns in tiles of 1 x 11, records in standard form (no codec list; the codecs are not
    what this is about); a rectangle inside its last two rows, read, and written over old records of two of its last three tiles"""
    import gridfour_amd
    import count_seams as S
    master = gridfour_amd.CodecMasterHip(codec_list=[], context=ctx)
    grid, tile = (2 ** 31 - 1, 11), (1, 11)
    assert B.tiles_of(grid, tile) == (0x7fffffff, 1)
    corner = Corner(grid, tile, (grid[0] - 3, 0), (3, 1))
    small_rect = (1, 2, 2, 7)
    rect = corner.rect(small_rect)
    assert rect[0] + rect[2] == grid[0] and corner.index([2])[0] == 0x7fffffff - 1
    elems, fills = ["int"], [-5]
    rng = np.random.default_rng(31)
    cells = rng.integers(1, 1000, (3, 11)).astype(np.int32)
    listed = np.array([2, 0])
    framed = S.frame_records(corner.index(listed), cells[listed].astype("<i4").view(np.uint8).reshape(2, 44))
    blob, offsets = framed.reshape(-1), np.arange(3, dtype=np.uint64) * framed.shape[1]
    blocks, st = master.read_block_dev(1, 11, grid, rect, blob, offsets, elems, fills=fills)
    assert (st == 0).all()
    want = B.block_from_tiles(corner.small, tile, small_rect, listed, cells[listed], -5)
    assert (want[0] == -5).all() and (want[1] != -5).all() and np.array_equal(blocks[0], want)
    new = rng.integers(1, 1000, (2, 7)).astype(np.int32)

    def encode(indices, tiles):
        n = len(indices)
        recs = S.frame_records(corner.index(indices), np.ascontiguousarray(tiles[0], "<i4").view(np.uint8).reshape(n, 44))
        return [r.tobytes() for r in recs], np.full((1, n), 255, np.uint8), np.zeros(n, np.int32)
    before = {int(t): [cells[t]] for t in listed}
    w_idx, w_recs, _, w_used, w_st = W.expected(encode, corner.small, tile, small_rect, [new], elems, fills, None, before)
    idx, got, used, wst = master.write_block_dev(1, 11, grid, rect, [new], elems, fills=fills, old=(blob, offsets))
    assert np.array_equal(idx, corner.index(w_idx)) and list(idx) == [0x7fffffff - 2, 0x7fffffff - 1]
    assert np.array_equal(wst, w_st) and (wst == 0).all() and np.array_equal(used, w_used) and got == w_recs


# ---------------------------------------------------------------- interpolation and render

def _far_rect():
    return CORNERS["the last four tiles"].rect(SMALL_RECT)


def _strip():
    """7 rows over the full width at the grid's last rows: wrap 1 and 2 have their wrapped windows"""
    return (GEBCO[0] - 7, 0, 7, GEBCO[1])


def _points(rng, spec, n):
    """interp_cases.fixed_points (written relative to the grid's size) and random points inside the block"""
    fr, fc = K.fixed_points(spec)
    r0, c0, nr, nc = spec.block
    rows = np.concatenate([fr, rng.uniform(r0, r0 + nr - 1, n), rng.uniform(r0 + 1.0, r0 + nr - 2.0, n)])
    cols = np.concatenate([fc, rng.uniform(c0, c0 + nc - 1, n), rng.uniform(max(c0, 1) + 1.0, c0 + nc - 3.0, n)])
    return rows, cols


def _lattice_over(spec, n_rows=37, n_cols=53):
    """a lattice from just outside the block's upper left corner to just beyond its lower right one"""
    r0, c0, nr, nc = spec.block
    c_lo, c_hi = (c0 - 0.7, c0 + nc - 0.4) if nc < 100 else (c0 + nc - 5.3, c0 + nc + 3.6)        # (the full-width strip: across the wrap seam)
    return (r0 - 0.6, c_lo, (nr + 0.9) / n_rows, (c_hi - c_lo) / n_cols, n_rows, n_cols)


FAR_CASES = [("corner", 0), ("strip", 0), ("strip", 1), ("strip", 2)]


@pytest.mark.parametrize("target", [R.VALUE, R.FIRST, R.SECOND])
@pytest.mark.parametrize("which,wrap", FAR_CASES, ids=["%s-wrap%d" % c for c in FAR_CASES])
def test_interpolation_at_the_far_corner(ctx, which, wrap, target):
    rng = np.random.default_rng(5000 + 10 * wrap + target)
    spec = R.Spec(GEBCO[0], GEBCO[1], _far_rect() if which == "corner" else _strip(), R.FLOAT, wrap=wrap, target=target,
                  row_spacing=0.37109375, col_spacing=1.9 / 3.0)
    block = K.random_block(rng, R.FLOAT, spec.block[2:])
    rows, cols = _points(rng, spec, 300)
    want = R.interp(spec, block, rows, cols)
    ok = want["status"] == R.OK
    assert ok.sum() > 300 and not np.isnan(want["z"][ok]).any() and {R.DECLINED, R.ERR_BOUNDS} <= set(want["status"].tolist())
    TI._same(TI.run_points(ctx, spec, block, rows, cols), want, (which, wrap, "points"))
    lattice = _lattice_over(spec)
    rows, cols = R.lattice_coords(*lattice)
    want = R.interp(spec, block, rows, cols)
    assert (want["status"] == R.OK).sum() > 500
    TI._same(TI.run_lattice(ctx, spec, block, lattice), want, (which, wrap, "lattice"))


@pytest.mark.parametrize("which,wrap", FAR_CASES, ids=["%s-wrap%d" % c for c in FAR_CASES])
def test_render_at_the_far_corner(ctx, which, wrap):
    """gf_block_render_lattice_dev with ETOPO1.cpt of tests/golden/palettes, normalised to the samples' range, and a light"""
    import gridfour_amd
    rng = np.random.default_rng(5100 + wrap)
    args = RC.cpt("ETOPO1.cpt", normalized=True, range_min=-128.0, range_max=128.0)
    model, pal = M.Palette(**args), gridfour_amd.Palette(ctx, **args)
    light = RC.LIGHTS["extract"]
    spec = R.Spec(GEBCO[0], GEBCO[1], _far_rect() if which == "corner" else _strip(), R.FLOAT, wrap=wrap, row_spacing=30.0, col_spacing=25.0)
    block = K.random_block(rng, R.FLOAT, spec.block[2:])
    lattice = _lattice_over(spec)
    rows, cols = R.lattice_coords(*lattice)
    want = M.render_points(spec, block, rows, cols, model, light)
    assert (want["status"] == R.OK).sum() > 500 and len(set(want["argb"].tolist())) > 50
    s, li = K.lib_spec(spec), RC.lib_light(light)
    got = TR._run_render(ctx, spec, block, rows.size, lambda d_block, o: ctx.render_lattice_dev(s, d_block, lattice, pal, o, li), ("argb", "shade", "status"))
    pal.close()
    TR._assert_render(got, want, (which, wrap))


@pytest.mark.parametrize("wrap", [0, 1])
def test_interpolation_on_the_largest_grid_the_checks_accept(ctx, wrap):
    """2^31 - 1 rows and columns (tests/test_interp_args.py: a block must lie inside an int32 grid); a 7 x 9 block at its last rows
    and columns, every output, both forms"""
    n = 2 ** 31 - 1
    rng = np.random.default_rng(5200 + wrap)
    spec = R.Spec(n, n, (n - 7, n - 9, 7, 9), R.FLOAT, wrap=wrap, target=R.SECOND, row_spacing=0.9, col_spacing=1.1)
    block = K.random_block(rng, R.FLOAT, (7, 9))
    rows, cols = _points(rng, spec, 300)
    want = R.interp(spec, block, rows, cols)
    assert (want["status"] == R.OK).sum() > 300
    TI._same(TI.run_points(ctx, spec, block, rows, cols), want, "points")
    lattice = _lattice_over(spec)
    rows, cols = R.lattice_coords(*lattice)
    want = R.interp(spec, block, rows, cols)
    assert (want["status"] == R.OK).sum() > 300
    TI._same(TI.run_lattice(ctx, spec, block, lattice), want, "lattice")
