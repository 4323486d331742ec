"""Cells read and B-spline interpolation at scattered points straight from GVRS file images (gf_file_read_points_elems[_dev],
gf_file_interp_points[_dev] behind GvrsFileHip; k_points_mark, k_points_rank, k_file_locate over a list, k_points_cells,
k_points_interp), held to the route through a block: every cell byte-equal to the whole-grid gf_file_read_block_elems_dev, every
interpolation output bit-equal to gf_block_interp_points_dev over that block, statuses included.  The reference's fifteen sample
files; the 299-tile image of the test-only writer at the wave, workgroup and bitmap-word seams; a grid of more than 32,768 tiles at
the chunk seam of k_points_rank; windows across tile seams under every wrap and element type; compressed tiles; max_tiles; damage,
one defect at a time; no points."""
import struct

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import _lib, GvrsFileHip, GvrsFileFacts, DeviceBuffer

import file_points_cases as K
import file_points_ref as R
import gvrs_file_build as B
import interp_ref as IR
from test_file_open import FACTS, sample_path
from test_gpu_file_read import image299, put

pytestmark = pytest.mark.gpu
OK, ERR_FORMAT, ERR_BOUNDS, ERR_ARG, ERR_CAPACITY = _lib.OK, _lib.ERR_FORMAT, _lib.ERR_BOUNDS, _lib.ERR_ARG, _lib.ERR_CAPACITY
INT_MIN = -2 ** 31


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


# ---- the route the library had before: the whole grid as a block, computed once per image and shared ----
def whole_grid(f, ctx, image=None, verify=True):
    blocks, status, _ = f.read_block_dev(ctx, (0, 0, f.grid[0], f.grid[1]), verify, image=image)
    return blocks, status


def fill_of(f, e):
    el = f.info["elems"][e]
    return el["fill_i"] if el["type"] in (0, 1) else np.float32(el["fill_f"])


def bad_tiles(status, e):
    return {int(t): int(status[e, t]) for t in np.nonzero(status[e])[0]}


def check_cells(f, ctx, rows, cols, whole, image=None, verify=True):
    """both forms against the block route; returns the device form's (values, status)"""
    rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    blocks, status = whole
    n_touched = R.cells_touched(f.grid, rows, cols).size
    got = None
    for read in (f.read_points_dev, f.read_points):
        values, st, touched = read(ctx, rows, cols, verify, image=image)
        assert touched == n_touched
        for e in range(f.n_elems):
            want_v, want_s = R.expected_cells(f.grid, blocks[e], fill_of(f, e), bad_tiles(status, e), rows, cols)
            assert values[e].dtype == blocks[e].dtype and values[e].tobytes() == want_v.tobytes(), (read.__name__, e)
            assert st[e].tolist() == want_s.tolist(), (read.__name__, e)
        got = got or (values, st)
    return got


def block_interp_dev(ctx, spec, block, rows, cols, cs):
    """gf_block_interp_points_dev over a block uploaded here: the dict GvrsHipContext.interp_points returns"""
    n, target = rows.size, int(spec["target"][0])
    names = ["z"] + (["zx", "zy", "normal"] if target >= 1 else []) + (["zxx", "zxy", "zyy"] if target >= 2 else [])
    bufs = [DeviceBuffer(ctx, block.nbytes + 16).upload(block), DeviceBuffer(ctx, n * 8 + 16).upload(rows), DeviceBuffer(ctx, n * 8 + 16).upload(cols)]
    d_cs = None if cs is None else DeviceBuffer(ctx, n * 8 + 16).upload(cs)
    out = {k: DeviceBuffer(ctx, n * (24 if k == "normal" else 8) + 16) for k in names}
    out["status"] = DeviceBuffer(ctx, n * 4 + 16)
    ctx.interp_points_dev(spec, bufs[0].ptr, n, bufs[1].ptr, bufs[2].ptr, {k: b.ptr for k, b in out.items()}, None if d_cs is None else d_cs.ptr)
    ctx.synchronize()
    res = {k: out[k].download(np.float64, n * (3 if k == "normal" else 1)) for k in names}
    res["status"] = out["status"].download(np.int32, n)
    if "normal" in res:
        res["normal"] = res["normal"].reshape(n, 3)
    for b in bufs + list(out.values()) + ([d_cs] if d_cs is not None else []):
        b.free()
    return res


def check_interp(f, ctx, e, rows, cols, whole, wrap=0, target=0, cs=None, image=None, verify=True, fringes=(None, None), touched=None):
    """both forms against gf_block_interp_points_dev over the whole-grid block of element e, with the one addition: a window over a
    tile whose element did not decode takes the status of the lowest-indexed such tile, and NaN.  Returns the device form's dict."""
    rows, cols = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(cols, np.float64)
    blocks, status = whole
    spec = f.points_spec(e, wrap=wrap, target=target, row_spacing=0.75, col_spacing=1.25, row_fringe=fringes[0], col_fringe=fringes[1])
    want = block_interp_dev(ctx, spec, blocks[e], rows, cols, cs)
    ref = R.spec_of(f.grid, wrap, fringes[0], fringes[1])
    bad = bad_tiles(status, e)
    if bad or touched is None:
        per_point = R.window_tiles(f.grid, ref, rows, cols)
        touched = len(set().union(*per_point)) if per_point else 0
        for i, tiles in enumerate(per_point):
            hit = [t for t in tiles if t in bad]
            if hit and want["status"][i] == OK:
                want["status"][i] = bad[hit[0]]
                for k in want:
                    if k != "status":
                        want[k][i] = np.nan
    got = None
    for read in (f.interp_points_dev, f.interp_points):
        res, n_touched = read(ctx, e, spec, rows, cols, cs, verify, image=image)
        assert n_touched == touched, read.__name__
        assert sorted(res) == sorted(want)
        assert res["status"].tolist() == want["status"].tolist(), read.__name__
        for k in res:
            if k != "status":
                assert IR.same_bits(res[k].ravel(), want[k].ravel()), (read.__name__, k)
        got = got or res
    return got


# ---- the fifteen sample files ----
@pytest.mark.parametrize("k", range(15))
def test_samples_every_cell(ctx, golden_dir, k):
    f = GvrsFileHip(sample_path(golden_dir, k))
    rows, cols = np.meshgrid(np.arange(f.grid[0]), np.arange(f.grid[1]), indexing="ij")
    order = np.random.default_rng(k).permutation(rows.size)
    whole = whole_grid(f, ctx)
    assert not whole[1].any()
    values, _ = check_cells(f, ctx, rows.ravel()[order], cols.ravel()[order], whole)
    back = np.empty_like(order)
    back[order] = np.arange(order.size)
    for e in range(f.n_elems):
        assert values[e][back].tobytes() == whole[0][e].tobytes()


@pytest.mark.parametrize("k", range(15))
def test_samples_interp_lattice(ctx, golden_dir, k):
    f = GvrsFileHip(sample_path(golden_dir, k))
    nr, nc = f.grid[:2]
    r, c = np.meshgrid(np.arange(-1.0, nr + 0.5, 0.5), np.arange(-1.0, nc + 0.5, 0.5), indexing="ij")
    rows, cols = r.ravel(), c.ravel()
    whole = whole_grid(f, ctx)
    touched = len(FACTS[k][7])                                            # the lattice covers the grid: every tile of it
    if rows.size < 5000:
        assert touched == R.windows_touched(f.grid, R.spec_of(f.grid), rows, cols).size
    for e in range(f.n_elems):
        for target in (0, 1, 2):
            res = check_interp(f, ctx, e, rows, cols, whole, target=target, touched=touched)
            assert (res["status"] == OK).any() and (res["status"] == 1).any()            # inside, and declined outside the fringe


# ---- the 299-tile image ----
@pytest.fixture(scope="module", params=[False, True], ids=["compact", "extended"])
def file299(request, ctx):
    image, named, want = image299(request.param)
    f = GvrsFileHip(image)
    whole = whole_grid(f, ctx)
    assert np.array_equal(whole[0][0], want) and not whole[1].any()
    return f, named, whole


def cell_of_tile(t, k=0):
    """cell k of tile t of the 299-tile grid (13 tiles across, 2 x 3 cells), inside the 45 x 37 grid"""
    r, c = divmod(t, 13)
    row, col = r * 2 + (k // 3) % 2, c * 3 + k % 3
    return min(row, 44), min(col, 36)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 4099])
def test_299_point_counts(ctx, file299, n):
    f, named, whole = file299
    rng = np.random.default_rng(n)
    rows, cols = rng.integers(0, 45, n), rng.integers(0, 37, n)
    if n > 1:
        outside = rng.integers(0, n, max(1, n // 9))                    # points outside the grid mixed in
        rows[outside], cols[outside] = rng.choice([-1, 45, -2 ** 31, 2 ** 31 - 1], outside.size), rng.integers(-2, 40, outside.size)
        dup = rng.integers(0, n, max(1, n // 5))                        # duplicates
        rows[dup], cols[dup] = rows[dup[0]], cols[dup[0]]
    values, st = check_cells(f, ctx, rows, cols, whole)
    if n >= 256:
        assert (st == ERR_ARG).any() and (values[0] == INT_MIN).any() and (values[0] != INT_MIN).any()
    drows, dcols = rng.uniform(-1.0, 45.5, n), rng.uniform(-1.0, 37.5, n)
    check_interp(f, ctx, 0, drows, dcols, whole, wrap=n % 3, target=n % 2 + 1)


def test_299_one_tile_and_a_tile_each(ctx, file299):
    f, named, whole = file299
    held = sorted(named)
    t = held[len(held) // 2]
    # every lane of a wave holds the same bitmap word and bit
    rows, cols = zip(*[cell_of_tile(t, k) for k in range(200)])
    values, _ = check_cells(f, ctx, rows, cols, whole)
    assert f.cells_tiles(rows, cols).tolist() == [t] and (values[0] != INT_MIN).all()
    # each of 64 consecutive points in a different tile, three waves of them, across the whole grid
    tiles = [(7 * i) % 299 for i in range(192)]
    rows, cols = zip(*[cell_of_tile(x, i) for i, x in enumerate(tiles)])
    check_cells(f, ctx, rows, cols, whole)
    assert len(set(tiles[:64])) == 64


@pytest.mark.parametrize("tiles", [(31, 32, 33), (63, 64), (31,), (32,), (0, 298), (95, 96, 127, 128, 160)])
def test_299_bitmap_word_seams(ctx, file299, tiles):
    f, named, whole = file299
    rows, cols = zip(*[cell_of_tile(t, k) for k in range(6) for t in tiles])
    check_cells(f, ctx, rows, cols, whole)
    assert f.cells_tiles(rows, cols).tolist() == list(tiles)


# ---- the chunk seam of k_points_rank ----
def test_rank_chunk_seam(ctx):
    chunk = K.RANK_CHUNK_WORDS
    grid = (364, 546, 2, 3)                                              # 182 x 182 = 33,124 tiles: 1,036 words of the bitmap
    across = 182
    seam = chunk * 32                                                    # the first tile of the second chunk's first word
    assert seam + 32 < across * across
    held = sorted({seam - 32, seam - 31, seam - 2, seam - 1, seam, seam + 1, seam + 30, seam + 31, seam - 32 - across, seam - across, seam + across}
                  | {seam - 40 + 3 * i for i in range(28)})
    rng = np.random.default_rng(33)
    cells = {t: rng.integers(-999, 999, (2, 3)).astype(np.int32) for t in held}
    records = {t: B.standard_record(t, [cells[t]]) for t in held}
    r0 = (seam - 40 - across) // across
    image, named = B.build_image(grid, [B.element("z", "int")], records, dir_rect=(r0, 0, 4, across))
    assert len(image) < 16384 and sorted(named) == held
    f = GvrsFileHip(image)
    whole = whole_grid(f, ctx)
    for t in held:
        r, c = divmod(t, across)
        assert np.array_equal(whole[0][0][r * 2:r * 2 + 2, c * 3:c * 3 + 3], cells[t])
    # points on both sides of the seam, in held and in absent tiles, and far in front of it
    absent = [t for t in (seam - 3, seam + 3, seam + 33, 0, 5, across * across - 1) if t not in held]
    assert len(absent) == 6
    tiles = held + absent
    rows = [(t // across) * 2 + k % 2 for k, t in enumerate(tiles)]
    cols = [(t % across) * 3 + k % 3 for k, t in enumerate(tiles)]
    values, st = check_cells(f, ctx, rows, cols, whole)
    assert not st.any() and (values[0][:len(held)] != INT_MIN).all() and (values[0][len(held):] == INT_MIN).all()
    assert f.cells_tiles(rows, cols).tolist() == sorted(set(tiles))
    # windows over the seam's tiles: tile rows 179 and 180 meet there
    r, c = divmod(seam, across)
    drows = np.array([r * 2 - 0.5, r * 2 + 0.5, r * 2 - 1.5, (r + 1) * 2 - 0.5] * 3)
    dcols = np.repeat([c * 3 - 0.5, c * 3 + 1.25, 0.25], 4)
    for wrap in (0, 1):
        check_interp(f, ctx, 0, drows, dcols, whole, wrap=wrap, target=1)


# ---- interpolation across seams ----
def test_299_windows_on_every_tile_corner(ctx, file299):
    f, named, whole = file299
    r, c = np.meshgrid(np.arange(0, 24) * 2 - 0.5, np.arange(0, 14) * 3 - 0.5, indexing="ij")
    rows, cols = r.ravel(), c.ravel()
    cs = np.random.default_rng(4).uniform(0.5, 2.0, rows.size)
    cs[::17] = 0.0                                                       # a zero spacing: GF_ERR_ARG for that point with target >= FIRST
    for wrap in (0, 1, 2):
        check_interp(f, ctx, 0, rows, cols, whole, wrap=wrap, target=2, cs=cs)
        res = check_interp(f, ctx, 0, rows, cols, whole, wrap=wrap, target=1)
        assert (res["status"] == OK).any()
    # the columns that a wrapped window takes from both ends
    cols = np.array([-0.5, 0.25, 37 - 0.75, -1.0, 36.5, 36.0, 35.0, 1.0] * 3)
    rows = np.repeat([0.25, 21.5, 43.75], 8)
    for wrap in (1, 2):
        res = check_interp(f, ctx, 0, rows, cols, whole, wrap=wrap, target=2)
        assert (res["status"] == OK).sum() >= 12


def image_mixed():
    """SHORT, INT, FLOAT and ICF elements over 2 x 3 tiles; every third tile absent; some cells fill"""
    grid = (13, 11, 2, 3)
    n_tile_rows, n_tile_cols = 7, 4
    rng = np.random.default_rng(8)
    shape = (n_tile_rows * 2, n_tile_cols * 3)
    planes = [rng.integers(-300, 300, shape).astype(np.int16), rng.integers(-10 ** 6, 10 ** 6, shape).astype(np.int32),
              rng.normal(0, 50, shape).astype(np.float32), rng.integers(-5000, 5000, shape).astype(np.int32)]
    planes[0][rng.integers(0, 12, shape) == 0] = -32768
    planes[1][3, :] = INT_MIN
    planes[2][:, 4] = np.float32(np.nan)
    planes[3][5, 5] = INT_MIN
    elements = [B.element("s", "short"), B.element("i", "int"), B.element("f", "float"), B.element("c", "icf", scale=8.0, offset=-3.0)]
    records = {}
    for t in range(n_tile_rows * n_tile_cols):
        if t % 7 == 3:
            continue
        r, c = divmod(t, n_tile_cols)
        records[t] = B.standard_record(t, [p[r * 2:r * 2 + 2, c * 3:c * 3 + 3] for p in planes])
    image, _ = B.build_image(grid, elements, records, order=sorted(records, key=lambda t: (t * 7) % 29))
    return image


def test_mixed_types_across_seams(ctx, golden_dir):
    f = GvrsFileHip(image_mixed())
    assert [e["type"] for e in f.info["elems"]] == [1, 0, 2, 3]
    whole = whole_grid(f, ctx)
    assert not whole[1].any()
    rows, cols = np.meshgrid(np.arange(13), np.arange(11), indexing="ij")
    check_cells(f, ctx, rows.ravel(), cols.ravel(), whole)
    r, c = np.meshgrid(np.arange(-0.5, 13.5, 0.5), np.arange(-0.75, 11.5, 0.75), indexing="ij")
    for e in range(4):
        for wrap in (0, 1, 2):
            res = check_interp(f, ctx, e, r.ravel(), c.ravel(), whole, wrap=wrap, target=2)
            ok = res["status"] == OK
            assert np.isnan(res["z"][ok]).any() and (~np.isnan(res["z"][ok])).any()      # fill cells read as NaN, as in a block
    f8 = GvrsFileHip(sample_path(golden_dir, 8))                          # the reference's own mixed types, per-point spacings
    whole8 = whole_grid(f8, ctx)
    r, c = np.meshgrid(np.arange(-0.5, 10.0, 0.25), np.arange(-0.5, 10.0, 0.25), indexing="ij")
    cs = np.linspace(0.5, 3.0, r.size)
    for e in range(f8.n_elems):
        check_interp(f8, ctx, e, r.ravel(), c.ravel(), whole8, wrap=1, target=1, cs=cs)


# ---- compressed tiles of the benchmark's size ----
def test_compressed_tiles(ctx):
    grid = (240, 300, 120, 150)
    y, x = np.meshgrid(np.arange(240), np.arange(300), indexing="ij")
    raster = np.rint(900 * np.sin(0.031 * x) * np.cos(0.023 * y) + 35 * np.sin(0.4 * (x + y))).astype(np.int32)
    image, idx, status, used = GvrsFileHip.write_image(ctx, GvrsFileFacts(grid, ["int"], codec_ids=["GvrsHuffman"]), [raster])
    assert not status.any() and len(image) < raster.nbytes // 2          # Huffman packings, not the standard form
    f = GvrsFileHip(image)
    whole = whole_grid(f, ctx)
    assert np.array_equal(whole[0][0], raster)
    rng = np.random.default_rng(1000)
    check_cells(f, ctx, rng.integers(0, 240, 1000), rng.integers(0, 300, 1000), whole)
    check_interp(f, ctx, 0, rng.uniform(-0.5, 239.5, 1000), rng.uniform(-0.5, 299.5, 1000), whole, target=2)
    # a track inside one tile decodes that tile alone
    _, _, touched = f.read_points_dev(ctx, np.arange(100), np.arange(100))
    assert touched == 1


# ---- max_tiles ----
def test_max_tiles(ctx, file299):
    f, named, whole = file299
    rows, cols = zip(*[cell_of_tile(t) for t in (3, 40, 41, 100, 250, 40)])
    n = 5
    for read in (f.read_points_dev, f.read_points):
        values, st, touched = read(ctx, rows, cols, max_tiles=n)[:3]
        assert touched == n and values[0].tolist() == [int(whole[0][0][r, c]) for r, c in zip(rows, cols)] and not st.any()
        out = read(ctx, rows, cols, max_tiles=n - 1, return_code=True)
        assert out[3] == ERR_CAPACITY and out[2] == n
        assert (out[0][0].view(np.uint8) == 0x7f).all() and (out[1].view(np.uint8) == 0x7f).all()
        if len(out) > 4:
            assert all((s == 0x7f).all() for s in out[4])               # the slack behind every output, to the last byte
        with pytest.raises(gridfour_amd.GvrsHipError) as e:
            read(ctx, rows, cols, max_tiles=n - 1)
        assert e.value.status == ERR_CAPACITY
    drows, dcols = np.array([0.5, 20.25, 43.0]), np.array([0.5, 18.5, 35.75])
    spec = f.points_spec(0, target=1)
    n = f.interp_tiles(spec, drows, dcols).size
    assert n == R.windows_touched(f.grid, R.spec_of(f.grid), drows, dcols).size
    for read in (f.interp_points_dev, f.interp_points):
        res, touched = read(ctx, 0, spec, drows, dcols, max_tiles=n)
        assert touched == n and res["status"].tolist() == [OK, OK, OK]
        res, touched, code = read(ctx, 0, spec, drows, dcols, max_tiles=n - 1, return_code=True)
        assert code == ERR_CAPACITY and touched == n
        assert all((a.view(np.uint8) == 0x7f).all() for a in res.values())
    # points that touch nothing need no room
    values, st, touched = f.read_points_dev(ctx, [-1, 45], [0, 0], max_tiles=0)
    assert touched == 0 and st.tolist() == [[ERR_ARG, ERR_ARG]] and values[0].tolist() == [INT_MIN, INT_MIN]
    res, touched = f.interp_points_dev(ctx, 0, spec, [np.nan, -3.0], [1.0, 1.0], max_tiles=0)
    assert touched == 0 and res["status"].tolist() == [ERR_ARG, 1] and np.isnan(res["z"]).all()


# ---- damage, one defect at a time ----
GRID_DMG = (12, 10, 3, 2)                                     # 4 x 5 tiles
BAD = 7                                                       # tile row 1, tile column 2: rows 3..5, columns 4..5


def image_dmg(checksums=True):
    rows, cols = np.meshgrid(np.arange(12), np.arange(10), indexing="ij")
    cells = (rows * 100 + cols + 1).astype(np.int32)
    records = {t: B.standard_record(t, [cells[(t // 5) * 3:(t // 5) * 3 + 3, (t % 5) * 2:(t % 5) * 2 + 2]], checksums) for t in range(20)}
    image, named = B.build_image(GRID_DMG, [B.element("z", "int")], records, order=[(t * 7) % 20 for t in range(20)], extended=True,
                                 checksums=checksums, between=lambda k: B.other_record(B.RECORD_METADATA, 16, seed=k) if k % 2 else b"")
    return image, named, cells


def entry_off_grid(image, named, f):
    at, w = B.entry_offset(image, f.info, BAD)
    return put(image, at, struct.pack("<q", named[BAD] + 4))


def tile_index_word(image, named, f):
    return B.refresh_record_crc(put(image, named[BAD], struct.pack("<i", BAD + 1)), named[BAD])


def body_byte(image, named, f):
    return put(image, named[BAD] + 9, bytes([image[named[BAD] + 9] ^ 0x40]))


@pytest.mark.parametrize("damage,want,verify", [(entry_off_grid, ERR_BOUNDS, True), (tile_index_word, ERR_FORMAT, True), (body_byte, ERR_FORMAT, True),
                                                (body_byte, OK, False)], ids=["entry", "tile index", "body byte", "body byte unverified"])
def test_damage(ctx, damage, want, verify):
    image, named, cells = image_dmg()
    f = GvrsFileHip(image)
    bad = damage(image, named, f)
    assert len(bad) == len(image) and bad != image
    whole = whole_grid(f, ctx, image=bad, verify=verify)
    st = np.zeros((1, 20), np.int32)
    st[0, BAD] = want
    assert whole[1].tolist() == st.tolist()                              # the status the block read reports for the tile
    rows, cols = np.meshgrid(np.arange(12), np.arange(10), indexing="ij")
    values, status = check_cells(f, ctx, rows.ravel(), cols.ravel(), whole, image=bad, verify=verify)
    in_bad = ((rows // 3) * 5 + cols // 2 == BAD).ravel()
    assert (status[0][in_bad] == want).all() and not status[0][~in_bad].any()
    assert np.array_equal(values[0][~in_bad], cells.ravel()[~in_bad])
    if want != OK:
        assert (values[0][in_bad] == INT_MIN).all()
    # windows: (1.5, 2.5) takes rows 0..3 and columns 1..4: of the damaged tile its corner cell (3, 4) alone
    drows = np.array([1.5, 1.5, 4.5, 9.5, 6.5, 1.5])
    dcols = np.array([2.5, 1.5, 4.5, 4.5, 7.5, 7.5])
    res = check_interp(f, ctx, 0, drows, dcols, whole, target=1, image=bad, verify=verify)
    assert res["status"].tolist() == [want, OK, want, OK, OK, OK]
    assert np.isnan(res["z"][[0, 2]]).all() == (want != OK) and not np.isnan(res["z"][[1, 3, 4, 5]]).any()


# ---- no points ----
def test_no_points(ctx, file299):
    f, named, whole = file299
    for read in (f.read_points_dev, f.read_points):
        values, st, touched = read(ctx, [], [])
        assert touched == 0 and values[0].size == 0 and st.shape == (1, 0)
    spec = f.points_spec(0)
    for read in (f.interp_points_dev, f.interp_points):
        res, touched = read(ctx, 0, spec, [], [])
        assert touched == 0 and res["z"].size == 0
