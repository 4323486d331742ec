"""A raster block written straight to tile records on the GPU (gf_block_write_elems_dev and its host form).  The expected bytes are
the numpy model of the cut, the tile cache's checks and the valid-data rule (tests/block_write_ref.py, pinned by
tests/test_block_write_ref.py) fed to the reference-pinned record writers tile_records_elems_dev / tile_records_elems; records,
offsets, tile indices, codec-used and statuses are compared exactly.  Shapes are the smallest at which each path can go wrong:
edge tiles that overhang the grid, rectangles that are aligned, unaligned, inside one tile, one cell, one row, one column, SHORT
rows whose two sides disagree modulo 4 and a tile with an odd cell count."""
import functools

import numpy as np
import pytest

import block_ref as B
import block_write_ref as W
import damage

pytestmark = pytest.mark.gpu
HUFFMAN, DEFLATE, NONE, CANON = 1, 2, 0, 3
LISTS = [(), (HUFFMAN,), (CANON,), (HUFFMAN, CANON)]
STANDARD = (HUFFMAN, DEFLATE, NONE, CANON)
F32 = np.float32
ICF = ("icf", 100.0, -5.0, -2**31, F32(np.nan))
FOUR = ["int", "short", "float", ICF]
SETS = {"int": ["int"], "short": ["short"], "four": FOUR}
GEOM = {"8x10": ((37, 53), (8, 10)), "32x32": ((70, 90), (32, 32))}


@pytest.fixture(scope="module")
def ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext()


@functools.lru_cache(maxsize=None)
def _master_cached(ctx, codecs):
    import gridfour_amd
    return gridfour_amd.CodecMasterHip(codec_list=list(codecs), context=ctx)


def _master(ctx, codecs):
    return _master_cached(ctx, tuple(codecs))


def raster(el, grid, seed=0):
    """smooth data (the codecs win on it), no fill values, inside every default range"""
    r, c = np.meshgrid(np.arange(grid[0]), np.arange(grid[1]), indexing="ij")
    k = W.kind_of(el)
    if k == "int":
        return (1000 + 3 * r + 2 * c + (r * c) // 7 + 17 * seed).astype(np.int32)
    if k == "short":
        return (-200 + 2 * r + c + (r + 2 * c) // 5 - 3 * seed).astype(np.int16)
    if k == "float":
        return (0.5 * r + 0.25 * c + 1.0 + seed).astype(F32)
    return (0.01 * (r * 3 + c) + 0.125 * seed).astype(F32)


def rasters(elems, grid, seed=0):
    return [raster(el, grid, seed) for el in elems]


def crop(rs, rect):
    r0, c0, nr, nc = rect
    return [np.ascontiguousarray(a[r0:r0 + nr, c0:c0 + nc]) for a in rs]


def rects_of(grid, tile):
    tr, tc = tile
    return [(0, 0, grid[0], grid[1]),                       # the whole grid
            (tr, tc, tr, 2 * tc) if grid[1] >= 3 * tc else (tr, tc, tr, tc),      # tile-aligned, interior
            (tr - 3, tc - 2, tr + 5, tc + 5),               # unaligned, touches 3 x 3 tiles
            (tr + 1, tc + 2, tr - 3, tc - 3),               # inside a single tile
            (tr + 2, 2 * tc - 1, 1, 1),                     # a single cell
            (1, tc + 1, grid[0] - 2, 1),                    # a one-column strip
            (2 * tr + 1, 3, 1, grid[1] - 4)]                # a one-row strip


def _encoder(master, tile, elems, checksums, fills, host=False):
    def encode(indices, tiles):
        if host:
            recs, used = master.tile_records_elems(tile[0], tile[1], indices, tiles, elems, checksums=checksums, fills=fills)
            return recs, used, np.zeros(len(recs), np.int32)
        return master.tile_records_elems_dev(tile[0], tile[1], indices, tiles, elems, checksums=checksums, fills=fills)
    return encode


def _check(master, grid, tile, rect, blocks, elems, fills=None, ranges=None, before=None, old=None, checksums=True, what=None, **kw):
    """write_block_dev against the model; returns (what came back, what was expected)"""
    want = W.expected(_encoder(master, tile, elems, checksums, fills), grid, tile, rect, blocks, elems, fills, ranges, before)
    got = master.write_block_dev(tile[0], tile[1], grid, rect, blocks, elems, fills=fills, ranges=ranges, old=old, checksums=checksums, **kw)
    _same(got, want, what or (grid, tile, rect))
    return got, want


def _same(got, want, what):
    idx, recs, used, st = got
    w_idx, w_recs, w_off, w_used, w_st = want
    assert np.array_equal(idx, w_idx), (what, idx, w_idx)
    assert np.array_equal(st, w_st), (what, st, w_st)
    assert np.array_equal(used, w_used), (what, np.argwhere(used != w_used)[:4])
    assert [len(r) for r in recs] == [len(r) for r in w_recs], what
    for j, (a, b) in enumerate(zip(recs, w_recs)):
        assert a == b, (what, "record", j, "of tile", int(idx[j]), "first differing byte",
                        int(np.argmax(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))))


# ---------------------------------------------------------------- 1. the geometry sweep

@functools.lru_cache(maxsize=None)
def _codecs_win_condition():
    """a condition on the INPUTS of the 32 x 32 cases, checked on the CPU with the oracle's encoders: on the first tile of the whole
    grid the INT element and the ICF codes pack shorter than their standard form under both integer codecs, and the FLOAT element
    has no codec in these lists, so a record of the four-element tile holds both shapes"""
    import oracle
    grid, tile = GEOM["32x32"]
    idx, tiles, pre = W.cut(grid, tile, (0, 0) + grid, rasters(FOUR, grid), FOUR)
    assert (pre == 0).all()
    for e in (0, 3):
        cells = np.ascontiguousarray(tiles[e][0], np.int32)
        for enc in (oracle.codec_huffman_encode, oracle.codec_canon_encode):
            pk = enc(0, tile[0], tile[1], cells)
            pk = pk[0] if isinstance(pk, tuple) else pk
            assert pk is not None and len(pk) < 4 * cells.size, (e, enc.__name__)
    return True


SWEEP = [(g, s, l) for g in GEOM for s in SETS for l in LISTS]


@pytest.mark.parametrize("geom,eset,codecs", SWEEP, ids=["%s-%s-%s" % (g, s, "".join(map(str, l)) or "none") for g, s, l in SWEEP])
def test_geometry_sweep(ctx, geom, eset, codecs):
    grid, tile = GEOM[geom]
    elems = SETS[eset]
    master = _master(ctx, codecs)
    rs = rasters(elems, grid)
    any_codec = any_std = False
    for rect in rects_of(grid, tile):
        for checksums in (True, False):
            got, _ = _check(master, grid, tile, rect, crop(rs, rect), elems, checksums=checksums)
            assert (got[3] == 0).all(), (rect, got[3])
            any_codec |= bool((got[2] != 255).any())
            any_std |= bool((got[2] == 255).any())
    if geom == "32x32" and eset == "four" and codecs:
        assert _codecs_win_condition() and any_codec and any_std
    if not codecs:
        assert not any_codec


SHORT_RECTS = [(0, 0, 23, 31), (3, 1, 9, 12), (3, 2, 9, 12), (4, 5, 7, 9), (6, 8, 3, 1), (1, 3, 20, 2), (11, 6, 1, 20)]


@pytest.mark.parametrize("codecs", [(), (HUFFMAN, CANON)], ids=["none", "13"])
def test_short_tiles_with_an_odd_cell_count(ctx, codecs):
    """tiles of 5 x 7 = 35 cells: every second tile starts at an address that is 2 modulo 4 (the padded standard form; the halfword
    path where block row and tile row disagree modulo 4); col0 odd and even, odd and even widths"""
    grid, tile = (23, 31), (5, 7)
    master = _master(ctx, codecs)
    for elems in (["short"], ["short", "int", "short"]):
        rs = rasters(elems, grid)
        for rect in SHORT_RECTS:
            _check(master, grid, tile, rect, crop(rs, rect), elems, fills=[-1] * len(elems))


# ---------------------------------------------------------------- 2. tiles without valid data

def test_tiles_without_data_are_declined(ctx):
    grid, tile = GEOM["8x10"]
    master = _master(ctx, (HUFFMAN, CANON))
    rect = (0, 0) + grid
    hole = (slice(8, 24), slice(20, 40))                            # tiles 8, 9, 14, 15 wholly inside
    holes = [8, 9, 14, 15]
    cases = [(["int"], [7], np.int32(7)), (["float"], [None], F32(np.nan)), (["float"], [0.0], F32(-0.0)), ([ICF], None, F32(np.nan))]
    for elems, fills, hole_value in cases:
        rs = rasters(elems, grid)
        full, _ = _check(master, grid, tile, rect, rs, elems, fills=fills)
        holed = [rs[0].copy()]
        holed[0][hole] = hole_value
        got, _ = _check(master, grid, tile, rect, holed, elems, fills=fills)
        idx, recs, used, st = got
        assert [int(i) for i in idx[st == W.DECLINED]] == holes and (st[st != W.DECLINED] == 0).all(), (elems, st)
        assert all(recs[j] == b"" for j in holes) and (used[:, holes] == 255).all()
        assert all(recs[j] == full[1][j] for j in range(30) if j not in holes), "the neighbours' bytes changed"
    # four elements, all fill in the hole: declined; one non-fill cell in one element keeps the tile
    fills = [7, -1, 0.0, None]
    rs = rasters(FOUR, grid)
    for a, f in zip(rs, (np.int32(7), np.int16(-1), F32(-0.0), F32(np.nan))):
        a[hole] = f
    got, _ = _check(master, grid, tile, rect, rs, FOUR, fills=fills)
    assert [int(i) for i in got[0][got[3] == W.DECLINED]] == holes
    for e, v in enumerate((np.int32(8), np.int16(0), F32(1e-45), F32(-5.0))):       # (-5.0 is the ICF's code 0)
        one = [a.copy() for a in rs]
        one[e][9, 23] = v                                           # a cell of tile 8
        got, _ = _check(master, grid, tile, rect, one, FOUR, fills=fills)
        assert [int(i) for i in got[0][got[3] == W.DECLINED]] == holes[1:] and got[3][8] == 0 and len(got[1][8]) > 0, e


# ---------------------------------------------------------------- 3. ranges

def test_default_ranges_accept_what_the_types_hold(ctx):
    grid, tile = (16, 20), (8, 10)
    master = _master(ctx, (CANON,))
    one = ("icf", 1.0, 0.0, 5, F32(np.nan))
    elems = ["int", "short", "float", one]
    rs = rasters(elems, grid)
    rs[0][0, 0], rs[0][0, 1] = 2**31 - 1, -2**31 + 1
    rs[1][0, 0], rs[1][0, 1] = 32767, -32767
    rs[2][0, :4] = [np.inf, -np.inf, F32(3.4028235e38), F32(-0.0)]
    rs[3][0, :3] = [F32(2147483648.0), F32(-2147483648.0), np.nan]   # saturate to INT_MAX / INT_MIN; the fill
    got, want = _check(master, grid, tile, (0, 0) + grid, rs, elems, fills=[0, 0, 0.0, None])
    assert (got[3] == 0).all()
    _, tiles, _ = W.cut(grid, tile, (0, 0) + grid, rs, elems, fills=[0, 0, 0.0, None])
    assert list(tiles[3][0][:3]) == [2**31 - 1, -2**31, 5]
    # INT_MIN is outside the INT default range unless it is the fill; -32768 likewise for SHORT
    rs[0][9, 12] = -2**31
    got, _ = _check(master, grid, tile, (0, 0) + grid, rs, elems, fills=[0, 0, 0.0, None])
    assert list(got[3]) == [0, 0, 0, W.ERR_BOUNDS]
    got, _ = _check(master, grid, tile, (0, 0) + grid, rs, elems, fills=[None, 0, 0.0, None])
    assert (got[3] == 0).all()


def test_custom_ranges_reject_one_tile(ctx):
    grid, tile = GEOM["8x10"]
    master = _master(ctx, (HUFFMAN, CANON))
    rect = (3, 4, 30, 45)
    rs = rasters(FOUR, grid)
    lo_hi = [(int(rs[0].min()), int(rs[0].max())), (int(rs[1].min()), int(rs[1].max())), (float(rs[2].min()), float(rs[2].max())),
             (float(rs[3].min()), float(rs[3].max()))]
    fills = [0, 0, 0.0, None]
    got, _ = _check(master, grid, tile, rect, crop(rs, rect), FOUR, fills=fills, ranges=lo_hi)
    assert (got[3] == 0).all()
    outside = [lo_hi[0][1] + 1, lo_hi[1][0] - 1, np.nextafter(F32(lo_hi[2][1]), F32(np.inf)), np.nextafter(F32(lo_hi[3][1]), F32(np.inf))]
    for e in range(4):
        bad = [a.copy() for a in rs]
        bad[e][17, 25] = outside[e]                                 # a cell of tile 14
        got, _ = _check(master, grid, tile, rect, crop(bad, rect), FOUR, fills=fills, ranges=lo_hi)
        assert [int(i) for i in got[0][got[3] != 0]] == [14] and got[3][list(got[0]).index(14)] == W.ERR_BOUNDS, e
        # the fill value outside the range is accepted (fills 0 / 0 / 0.0 / NaN all lie outside these ranges)
        ok = [a.copy() for a in rs]
        ok[e][17, 25] = (0, 0, 0.0, np.nan)[e]
        got, _ = _check(master, grid, tile, rect, crop(ok, rect), FOUR, fills=fills, ranges=lo_hi)
        assert (got[3] == 0).all(), e
    # a NaN in a FLOAT element whose fill is 0, default ranges
    bad = [a.copy() for a in rs]
    bad[2][17, 25] = np.nan
    got, _ = _check(master, grid, tile, rect, crop(bad, rect), FOUR, fills=fills)
    assert [int(i) for i in got[0][got[3] != 0]] == [14] and (got[3][got[3] != 0] == W.ERR_BOUNDS).all()
    # out of range and no valid data elsewhere in the tile: ERR_BOUNDS comes before DECLINED
    lone = [np.full(grid, f, a.dtype) for a, f in zip(rs, (0, 0, 0.0, np.nan))]
    lone[0][17, 25] = lo_hi[0][1] + 1
    got, _ = _check(master, grid, tile, rect, crop(lone, rect), FOUR, fills=fills, ranges=lo_hi)
    assert set(got[3]) == {W.DECLINED, W.ERR_BOUNDS} and got[3][list(got[0]).index(14)] == W.ERR_BOUNDS


# ---------------------------------------------------------------- 4. read-modify-write

def _blob(records):
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    return np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8)[:int(off[-1])], off


def test_read_modify_write(ctx):
    grid, tile = GEOM["8x10"]
    codecs = (HUFFMAN, CANON)
    master = _master(ctx, codecs)
    fills = [0, None, 0.0, None]            # (SHORT: -32768, the one fill that survives a packing: TileElementShort.decode reads the null code as it)
    whole = (0, 0) + grid
    rs1 = rasters(FOUR, grid)
    (idx1, recs1, _, st1), _ = _check(master, grid, tile, whole, rs1, FOUR, fills=fills)
    assert (st1 == 0).all() and idx1.size == 30
    _, tiles1, _ = W.cut(grid, tile, whole, rs1, FOUR, fills=fills)
    (_, recs0, _, st0), _ = _check(master, grid, tile, whole, rasters(FOUR, grid, seed=5), FOUR, fills=fills)      # an earlier state of the file
    rect = (5, 7, 20, 30)                                           # tile rows 0..3, tile columns 0..3; tiles 7, 8, 13, 14 wholly covered
    widx = W.tile_indices(grid, tile, rect)
    assert widx.size == 16
    dropped = [0, 21]                                               # partly covered tiles the file does not hold yet
    order = [int(t) for t in np.random.default_rng(3).permutation(30) if int(t) not in dropped]
    old_recs = [recs0[9]] + [recs1[t] for t in order]               # tile 9 twice: the later record must win
    before = {t: [tiles1[e][t] for e in range(4)] for t in order}
    rs2 = rasters(FOUR, grid, seed=9)
    blocks = crop(rs2, rect)
    got, want = _check(master, grid, tile, rect, blocks, FOUR, fills=fills, before=before, old=_blob(old_recs))
    assert (got[3] == 0).all()
    # the file read back, new records listed last: the raster with the rectangle replaced; tiles 0 and 21 hold fill outside it
    as_int = ["int", "short", "float", "int"]
    blob, off = _blob(old_recs + got[1])
    back, st = master.read_block_dev(tile[0], tile[1], grid, whole, blob, off, as_int, fills=fills[:3] + [ICF[3]])
    assert (st == 0).all()
    codes1, _ = W.icf_convert(rs1[3], ICF)
    codes2, _ = W.icf_convert(rs2[3], ICF)
    for e, (a1, a2) in enumerate(zip(rs1[:3] + [codes1], rs2[:3] + [codes2])):
        exp = np.asarray(a1).copy()
        f = W.fill_of(as_int[e], (fills[:3] + [ICF[3]])[e])
        for t in dropped:
            r, c = divmod(t, 6)
            exp[r * 8:(r + 1) * 8, c * 10:(c + 1) * 10] = f
        exp[5:25, 7:37] = np.asarray(a2)[5:25, 7:37]
        assert np.array_equal(np.ascontiguousarray(back[e]).view(np.uint32 if e == 2 else back[e].dtype),
                              np.ascontiguousarray(exp.astype(back[e].dtype)).view(np.uint32 if e == 2 else back[e].dtype)), e
    # an old record of a PARTLY covered tile damaged: that tile alone gets the decoder's status and no record
    k = order.index(2) + 1
    hurt = list(old_recs)
    hurt[k] = damage._flip(hurt[k], 8 * (len(hurt[k]) // 2))
    blob, off = _blob(hurt)
    _, _, dst = master.record_blob_elems_dev(tile[0], tile[1], blob, off, as_int)
    bad = [int(s) for s in dst[:, k] if s != 0]
    assert bad, "the damage was not noticed by the decoder"
    b2 = dict(before)
    b2[2] = bad[0]
    got2, _ = _check(master, grid, tile, rect, blocks, FOUR, fills=fills, before=b2, old=(blob, off))
    j = list(got2[0]).index(2)
    assert got2[3][j] == bad[0] and got2[1][j] == b"" and (np.delete(got2[3], j) == 0).all()
    assert [r for i, r in enumerate(got2[1]) if i != j] == [r for i, r in enumerate(got[1]) if i != j]
    # ... of a WHOLLY covered tile: nothing changes
    k = order.index(13) + 1
    hurt = list(old_recs)
    hurt[k] = damage._flip(hurt[k], 8 * (len(hurt[k]) // 2))
    got3 = master.write_block_dev(tile[0], tile[1], grid, rect, blocks, FOUR, fills=fills, old=_blob(hurt))
    _same(got3, want, "damaged record of a wholly covered tile")


# ---------------------------------------------------------------- 5. capacity

def test_capacity_whole_records_only(ctx):
    grid, tile = GEOM["8x10"]
    master = _master(ctx, (HUFFMAN, CANON))
    elems, fills = ["int", "short"], [0, 0]
    rect = (6, 8, 12, 14)                                           # 3 x 3 tiles
    rs = rasters(elems, grid)
    rs[0][8:16, 10:20] = 0
    rs[1][8:16, 10:20] = 0                                          # the middle tile: no data, a record of length 0
    blocks = crop(rs, rect)
    (idx, recs, used, st), want = _check(master, grid, tile, rect, blocks, elems, fills=fills)
    assert list(st) == [0, 0, 0, 0, W.DECLINED, 0, 0, 0, 0]
    w_off = want[2]
    flat = np.frombuffer(b"".join(recs), np.uint8)
    total = int(w_off[-1])
    for cap in sorted({int(o) + d for o in w_off for d in (-1, 0, 1) if int(o) + d >= 0}):
        g_idx, blob, off, g_used, g_st = master.write_block_dev(tile[0], tile[1], grid, rect, blocks, elems, fills=fills, blob_cap=cap, raw=True)
        assert np.array_equal(off, w_off) and int(off[-1]) == total, cap       # offsets[n_out] reports the need
        assert np.array_equal(g_st, st) and np.array_equal(g_used, used) and np.array_equal(g_idx, idx)
        for j in range(9):
            a, b = int(off[j]), int(off[j + 1])
            if b <= cap:
                assert np.array_equal(blob[a:b], flat[a:b]), (cap, j)
            else:
                assert (blob[a:min(b, blob.size)] == 0xA5).all(), (cap, j, "a record that does not fit was written in part")
        assert (blob[min(cap, blob.size):] == 0xA5).all(), (cap, "a byte at or behind blob_cap was written")


# ---------------------------------------------------------------- 6. the host form

def test_host_form(ctx):
    grid, tile = GEOM["32x32"]
    fills = [0, None, 0.0, None]            # (SHORT: -32768, the one fill that survives a packing: TileElementShort.decode reads the null code as it)
    rect = (0, 0) + grid
    rs = rasters(FOUR, grid)
    rs[0][32:64, 32:64], rs[1][32:64, 32:64], rs[2][32:64, 32:64], rs[3][32:64, 32:64] = 0, -32768, 0.0, np.nan   # tile 4: no data
    dev = _master(ctx, (HUFFMAN, CANON))
    got, want = _check(dev, grid, tile, rect, rs, FOUR, fills=fills)
    host = dev.write_block(tile[0], tile[1], grid, rect, rs, FOUR, fills=fills)
    _same(host, want, "host form, device list")
    assert list(host[3]) == [0, 0, 0, 0, W.DECLINED, 0, 0, 0, 0]
    # the standard list (CodecDeflate, CodecFloat): the host writer's bytes on the model's tiles
    std = _master(ctx, STANDARD)
    want = W.expected(_encoder(std, tile, FOUR, True, fills, host=True), grid, tile, rect, rs, FOUR, fills)
    got = std.write_block(tile[0], tile[1], grid, rect, rs, FOUR, fills=fills)
    _same(got, want, "host form, standard list")
    assert (got[2][:, 4] == 255).all() and {int(u) for u in got[2][2]} == {2, 255}                # CodecFloat packed the FLOAT element
    blob, off = _blob([r for r in got[1] if r])                                       # (tile 4 has no record: it reads as fill)
    back, st = std.read_block(tile[0], tile[1], grid, rect, blob, off, FOUR, fills=fills)
    assert st.shape == (4, 8) and (st == 0).all()
    for e in range(3):
        assert np.array_equal(back[e].view(np.uint32 if e == 2 else back[e].dtype), rs[e].view(np.uint32 if e == 2 else rs[e].dtype)), e
    codes, _ = W.icf_convert(rs[3], ICF)
    with np.errstate(invalid="ignore"):
        exp = np.where(codes == ICF[3], F32(np.nan), codes.astype(F32) / F32(ICF[1]) + F32(ICF[2])).astype(F32)
    assert np.array_equal(back[3].view(np.uint32), exp.view(np.uint32))
    # a rejected tile: every array is filled in and the call returns the first negative status; too small a blob: ERR_CAPACITY
    bad = [a.copy() for a in rs]
    bad[0][1, 1] = 5000
    rc, idx, recs, used, st, off = std.write_block(tile[0], tile[1], grid, rect, bad, FOUR, fills=fills, ranges=[(0, 4000), None, None, None],
                                                   return_code=True)
    assert rc == W.ERR_BOUNDS and list(st) == [W.ERR_BOUNDS, 0, 0, 0, W.DECLINED, 0, 0, 0, 0] and recs[0] == b"" and recs[1:] == got[1][1:]
    import gridfour_amd
    for m, w in ((dev, host), (std, got)):
        total = sum(len(r) for r in w[1])
        rc, idx, recs, used, st, off = m.write_block(tile[0], tile[1], grid, rect, rs, FOUR, fills=fills, blob_cap=total - 1, return_code=True)
        assert rc == gridfour_amd.ERR_CAPACITY and int(off[-1]) == total
        rc, idx, recs, used, st, off = m.write_block(tile[0], tile[1], grid, rect, rs, FOUR, fills=fills, blob_cap=total, return_code=True)
        assert rc == 0 and recs == w[1]


# ---------------------------------------------------------------- 7. one context, several calls

def test_context_reuse(ctx):
    grid, tile = GEOM["8x10"]
    master = _master(ctx, (HUFFMAN, CANON))
    fills = [0, -1, 0.0, None]
    whole = (0, 0) + grid
    rs = rasters(FOUR, grid)
    rect = (5, 7, 20, 30)

    def write():
        return master.write_block_dev(tile[0], tile[1], grid, whole, rs, FOUR, fills=fills)

    first = write()
    old = _blob(first[1])
    _, tiles, _ = W.cut(grid, tile, whole, rs, FOUR, fills=fills)
    as_int = ["int", "short", "float", "int"]

    def read():
        return master.read_block_dev(tile[0], tile[1], grid, rect, old[0], old[1], as_int, fills=fills[:3] + [ICF[3]])

    def rmw():
        return master.write_block_dev(tile[0], tile[1], grid, rect, crop(rasters(FOUR, grid, seed=2), rect), FOUR, fills=fills, old=old)

    def encode():
        return master.tile_records_elems_dev(tile[0], tile[1], first[0], tiles, as_int, fills=fills)

    ref_read, ref_rmw, ref_enc = read(), rmw(), encode()
    assert ref_enc[0] == first[1]
    for order in ((read, write, encode, rmw), (rmw, encode, write, read), (encode, rmw, read, write)):
        for f in order:
            got = f()
            if f is read:
                assert all(np.array_equal(a.view(np.uint32 if a.dtype == F32 else a.dtype), b.view(np.uint32 if b.dtype == F32 else b.dtype))
                           for a, b in zip(got[0], ref_read[0])) and np.array_equal(got[1], ref_read[1])
            elif f is encode:
                assert got[0] == ref_enc[0] and np.array_equal(got[1], ref_enc[1]) and np.array_equal(got[2], ref_enc[2])
            else:
                w = first if f is write else ref_rmw
                assert np.array_equal(got[0], w[0]) and got[1] == w[1] and np.array_equal(got[2], w[2]) and np.array_equal(got[3], w[3])
