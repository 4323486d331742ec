"""Grid blocks on the GPU (gf_block_from_tiles_dev, gf_tiles_from_block_dev, gf_block_read_elems_dev and its host form): the
reference's own sample files read as blocks; the gather and the cut against the numpy model of tests/block_ref.py at the smallest
shapes at which each path of the row copy can go wrong; absent, failed and duplicate tiles; records of three elements read into
blocks against gf_tile_record_decode_batch_elems_dev on the same bytes; a block read beside a decode on one context from two
threads, and the gather replayed from a hipGraph."""
import ctypes as C
import threading

import numpy as np
import pytest

import block_ref as B
import test_gpu_graph as TG
import test_gpu_records_elems as RE
from test_gpu_records_dev import _flip, _frame_elems, _shifted
from test_gpu_records_dev import ctx, master5      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NULL = -2**31
INT, SHORT, FLOAT, ICF = 0, 1, 2, 3
GUARD = 0xA5A5A5A5                                  # the guard bands' and the "before" tiles' sentinel (0xA5A5 for 2-byte items)


def _sentinel(dtype):
    dtype = np.dtype(dtype)
    return np.array([GUARD & (0xffff if dtype.itemsize == 2 else 0xffffffff)], np.uint16 if dtype.itemsize == 2 else np.uint32).view(dtype)[0]


class Guarded:
    """n items of dtype in device memory with a guard band of `band` items of the sentinel on both sides"""

    def __init__(self, ctx, n, dtype, band=64):
        import gridfour_amd
        self.n, self.dtype, self.band = n, np.dtype(dtype), band
        self.sentinel = _sentinel(dtype)
        self.buf = gridfour_amd.DeviceBuffer(ctx, (n + 2 * band) * self.dtype.itemsize)
        self.buf.upload(np.full(n + 2 * band, self.sentinel, self.dtype))
        self.ptr = C.c_void_p(self.buf.ptr.value + band * self.dtype.itemsize)

    def put(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.size == self.n and a.dtype.itemsize == self.dtype.itemsize
        self.buf.upload(a, self.band * self.dtype.itemsize)
        return self

    def get(self):
        """the items; the guard bands must be intact"""
        all_ = self.buf.download(self.dtype, self.n + 2 * self.band)
        assert (all_[:self.band] == self.sentinel).all() and (all_[self.band + self.n:] == self.sentinel).all(), "guard band overwritten"
        return all_[self.band:self.band + self.n]

    def free(self):
        self.buf.free()


def _i32(ctx, a):
    import gridfour_amd
    a = np.ascontiguousarray(a, np.int32)
    buf = gridfour_amd.DeviceBuffer(ctx, a.nbytes + 16)
    return buf.upload(a) if a.size else buf


def _gather(ctx, grid, tile, rect, dtype, fill_bits, indices, tiles, status=None, bands=(64, 64)):
    """gf_block_from_tiles_dev on uploaded tiles; the block [n_rows, n_cols]"""
    tiles = np.ascontiguousarray(tiles, dtype)
    d_tiles = Guarded(ctx, max(tiles.size, 1), dtype, bands[0])
    if tiles.size:
        d_tiles.put(tiles)
    d_block = Guarded(ctx, rect[2] * rect[3], dtype, bands[1])
    d_idx = _i32(ctx, indices)
    d_st = None if status is None else _i32(ctx, status)
    try:
        ctx.block_from_tiles_dev(tuple(grid) + tuple(tile), rect, SHORT if np.dtype(dtype).itemsize == 2 else INT, fill_bits, len(indices),
                                 d_idx.ptr, d_tiles.ptr, d_block.ptr, None if d_st is None else d_st.ptr)
        ctx.synchronize()
        d_tiles.get()
        return d_block.get().reshape(rect[2], rect[3])
    finally:
        for b in (d_tiles, d_block, d_idx) + (() if d_st is None else (d_st,)):
            b.free()


def _cut(ctx, grid, tile, rect, dtype, fill_bits, block, indices, before=None, bands=(64, 64)):
    """gf_tiles_from_block_dev; (tiles [n, cells], status).  before: what the tiles hold (keep_outside), else the sentinel."""
    cells = tile[0] * tile[1]
    d_tiles = Guarded(ctx, len(indices) * cells, dtype, bands[0])
    if before is not None:
        d_tiles.put(before)
    d_block = Guarded(ctx, rect[2] * rect[3], dtype, bands[1]).put(np.ascontiguousarray(block, dtype))
    d_idx = _i32(ctx, indices)
    d_st = _i32(ctx, np.full(len(indices), 77, np.int32))
    try:
        ctx.tiles_from_block_dev(tuple(grid) + tuple(tile), rect, SHORT if np.dtype(dtype).itemsize == 2 else INT, fill_bits, d_block.ptr,
                                 len(indices), d_idx.ptr, d_tiles.ptr, d_st.ptr, keep_outside=before is not None)
        ctx.synchronize()
        d_block.get()
        return d_tiles.get().reshape(len(indices), cells), d_st.download(np.int32, len(indices))
    finally:
        for b in (d_tiles, d_block, d_idx, d_st):
            b.free()


# ---------------------------------------------------------------- 1. the reference's own bytes

SAMPLES = [s for s in RE.SAMPLES if s[0][:8] in ("Sample02", "Sample03", "Sample06", "Sample07", "Sample08", "Sample09", "Sample10", "Sample11",
                                                "Sample12")]


def _rects(grid, tile):
    return [(0, 0, grid, grid),                                  # the whole grid
            (3, 4, 1, 1),                                        # one cell
            (1, 1, tile - 2, tile - 2),                          # inside one tile
            (tile - 2, tile - 2, 4, 4),                          # across the corner where the four tiles meet
            (0, 3, grid, grid - 4),                              # an odd col0
            (grid - 3, grid - 5, 3, 5)]                          # the last row and the last column


def _ramp_block(grid, rect, dtype):
    r0, c0, nr, nc = rect
    return ((np.arange(r0, r0 + nr)[:, None] * grid + np.arange(c0, c0 + nc)[None, :]) - 1).astype(dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name,codecs,tile,grid,elems,verify,fills", SAMPLES, ids=[c[0][:8] for c in SAMPLES])
def test_reference_samples_as_blocks(golden_dir, ctx, name, codecs, tile, grid, elems, verify, fills):
    import gridfour_amd
    assert len(SAMPLES) == 9
    master = gridfour_amd.CodecMasterHip(context=ctx) if codecs is None else gridfour_amd.CodecMasterHip(codec_list=codecs, context=ctx)
    blob, offsets, want_idx, _ = RE._sample_blob(golden_dir, name)
    dtypes = [RE._np_dtype(el) for el in elems]
    for rect in _rects(grid, tile):
        blocks, st = master.read_block_dev(tile, tile, (grid, grid), rect, blob, offsets, elems, verify_checksums=verify)
        assert st.shape == (len(elems), 4) and (st == 0).all(), (rect, st)
        for e, dt in enumerate(dtypes):
            assert blocks[e].dtype == dt and blocks[e].shape == (rect[2], rect[3])
            # (no padding of an edge tile, no fill: every cell of the grid is in the file)
            assert np.array_equal(_bits(blocks[e]), _bits(_ramp_block(grid, rect, dt))), (name, rect, e)
    # one record left out of the offsets: the record in front of it spans its bytes, its quarter of the grid reads as fill
    out = 2
    fewer = np.delete(offsets, out)
    blocks, st = master.read_block_dev(tile, tile, (grid, grid), (0, 0, grid, grid), blob, fewer, elems, verify_checksums=verify)
    assert st.shape == (len(elems), 3) and (st == 0).all(), st
    per_row = -(-grid // tile)
    tr, tc = divmod(want_idx[out], per_row)
    for e, dt in enumerate(dtypes):
        want = _ramp_block(grid, (0, 0, grid, grid), dt)
        want[tr * tile:(tr + 1) * tile, tc * tile:(tc + 1) * tile] = np.asarray(fills[e], dt)
        assert np.array_equal(_bits(blocks[e]), _bits(want)), (name, e)


# ---------------------------------------------------------------- 2. the gather and the cut against numpy

SHAPES = [((5, 5), (10, 10)),            # baseline
          ((6, 6), (10, 10)),            # partial edge tiles
          ((7, 9), (23, 31)),            # nothing 16-byte aligned
          ((40, 60), (100, 200)),        # rows shorter than a wave
          ((3, 300), (7, 650)),          # a row wider than the workgroup
          ((1, 5000), (3, 11000))]       # a row of more than four 16-byte pieces per lane of the whole workgroup: the piece loop runs twice


def _rect_list(grid):
    """the whole grid, the last cell, and eight rectangles with col0 = 0 .. 7 and n_cols of every residue modulo 8 (the widest that
    fits: they cross tile boundaries wherever the grid has any), over varying rows"""
    gr, gc = grid
    rects = [(0, 0, gr, gc), (gr - 1, gc - 1, 1, 1)]
    for k in range(8):
        n = 8 - k
        n += (gc - k - n) // 8 * 8
        r0 = (3 * k + 1) % gr
        rects.append((r0, k, max(1, (gr - r0) * (k + 1) // 8), n))
    assert {r[1] % 8 for r in rects[2:]} == set(range(8)) and {r[3] % 8 for r in rects[2:]} == set(range(8))
    assert all(r[0] + r[2] <= gr and r[1] + r[3] <= gc for r in rects)
    return rects


@pytest.mark.parametrize("item", [2, 4])
@pytest.mark.parametrize("tile,grid", SHAPES, ids=["%dx%d" % t for t, _ in SHAPES])
def test_gather_and_cut_equal_the_model(ctx, tile, grid, item):
    dtype = np.uint16 if item == 2 else np.uint32
    sentinel = GUARD & (0xffff if item == 2 else 0xffffffff)
    fill = 0x8000 if item == 2 else 0x80000000
    rng = np.random.default_rng(tile[0] * 1000 + tile[1] + item)
    nrt, nct = B.tiles_of(grid, tile)
    nt, cells = nrt * nct, tile[0] * tile[1]
    order = rng.permutation(nt)
    tiles = rng.integers(0, 2**(8 * item) - 1, (nt, cells)).astype(dtype)
    tiles[tiles == sentinel] = 1
    for k, rect in enumerate(_rect_list(grid)):
        bands = (64 + k % 4, 64 + (k // 2) % 4)                 # the arrays themselves at several alignments
        got = _gather(ctx, grid, tile, rect, dtype, fill, order, tiles, bands=bands)
        assert np.array_equal(got, B.block_from_tiles(grid, tile, rect, order, tiles, fill)), ("gather", rect)
        block = rng.integers(0, 2**(8 * item) - 1, (rect[2], rect[3])).astype(dtype)
        block[block == sentinel] = 2
        cut, st = _cut(ctx, grid, tile, rect, dtype, fill, block, order, bands=bands)
        assert (st == 0).all()
        assert np.array_equal(cut, B.tiles_from_block(grid, tile, rect, block, order, fill)), ("cut", rect)
        before = np.full((nt, cells), sentinel, dtype)
        kept, st = _cut(ctx, grid, tile, rect, dtype, fill, block, order, before=before, bands=bands)
        want = B.tiles_from_block(grid, tile, rect, block, order, fill, before=before)
        assert (st == 0).all() and np.array_equal(kept, want), ("cut, keep_outside", rect)
        assert (kept == sentinel).sum() == nt * cells - rect[2] * rect[3]       # cells outside the rectangle still hold the sentinel
        assert np.array_equal(_gather(ctx, grid, tile, rect, dtype, fill, order, cut, bands=bands), block), ("gather(cut(x))", rect)


def test_float_bits_survive(ctx):
    """NaN payloads, -0.0 and a denormal through the cut and the gather: cells move as bits"""
    tile, grid, rect = (7, 9), (23, 31), (2, 3, 20, 27)
    rng = np.random.default_rng(5)
    block = rng.standard_normal((rect[2], rect[3])).astype(np.float32).view(np.uint32)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000], np.uint32)
    block.reshape(-1)[::5] = special[np.arange(block.reshape(-1)[::5].size) % 7]      # NaNs with payloads, -0.0, denormals, an infinity
    fill = 0x7fc0beef                                            # a NaN with a payload of its own
    nrt, nct = B.tiles_of(grid, tile)
    order = np.arange(nrt * nct)[::-1]
    for elem_type in (FLOAT, ICF):
        d_block = Guarded(ctx, block.size, np.uint32).put(block)
        d_tiles = Guarded(ctx, order.size * 63, np.uint32)
        d_back = Guarded(ctx, block.size, np.uint32)
        d_idx = _i32(ctx, order)
        g = grid + tile
        ctx.tiles_from_block_dev(g, rect, elem_type, fill, d_block.ptr, order.size, d_idx.ptr, d_tiles.ptr)
        ctx.block_from_tiles_dev(g, rect, elem_type, fill, order.size, d_idx.ptr, d_tiles.ptr, d_back.ptr)
        ctx.synchronize()
        cut = d_tiles.get().reshape(order.size, 63)
        assert np.array_equal(cut, B.tiles_from_block(grid, tile, rect, block, order, fill))
        assert (cut == fill).sum() == cut.size - block.size
        assert np.array_equal(d_back.get().reshape(block.shape), block)
        for b in (d_block, d_tiles, d_back, d_idx):
            b.free()


# ---------------------------------------------------------------- 3. absent, failed and duplicate tiles

@pytest.mark.parametrize("item", [2, 4])
def test_absent_failed_and_duplicate_tiles(ctx, item):
    dtype = np.int16 if item == 2 else np.int32
    tile, grid = (6, 6), (10, 10)                                # 2 x 2 tiles, the last row and column of tiles reach beyond the grid
    fill = -32768 if item == 2 else NULL
    rng = np.random.default_rng(item)
    cells = 36
    # list entry: tile index, status
    entries = [(3, 0), (0, 0), (-1, 0), (4, 0), (1, 0), (0, 0), (2, -1), (2**31 - 1, 0), (-2**31, 0)]
    idx = np.array([i for i, _ in entries], np.int32)
    st = np.array([s for _, s in entries], np.int32)
    tiles = rng.integers(-30000, 30000, (len(entries), cells)).astype(dtype)
    whole = (0, 0, 10, 10)
    got = _gather(ctx, grid, tile, whole, dtype, fill, idx, tiles, status=st)
    want = B.block_from_tiles(grid, tile, whole, idx, tiles, fill, ok=st == 0)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:6, :6], tiles[5].reshape(6, 6))                  # tile 0 is listed twice: the later entry's values
    assert not np.array_equal(tiles[1], tiles[5])
    assert (got[6:, :6] == fill).all()                                          # tile 2: GF_ERR_FORMAT
    assert np.array_equal(got[6:, 6:], tiles[0].reshape(6, 6)[:4, :4])          # tile 3, cut at the grid's edge
    # without the statuses the failed tile's cells are delivered; a later failed entry of a tile hides an earlier good one
    assert np.array_equal(_gather(ctx, grid, tile, whole, dtype, fill, idx, tiles), B.block_from_tiles(grid, tile, whole, idx, tiles, fill))
    st2 = st.copy()
    st2[5] = -2
    got2 = _gather(ctx, grid, tile, whole, dtype, fill, idx, tiles, status=st2)
    assert (got2[:6, :6] == fill).all() and np.array_equal(got2[:, 6:], got[:, 6:])
    # a rectangle inside tile 1 alone: the entries of tiles 0, 2, 3 lie outside the rectangle of tiles and change nothing
    rect = (1, 7, 4, 3)
    only = _gather(ctx, grid, tile, rect, dtype, fill, idx, tiles, status=st)
    assert np.array_equal(only, tiles[4].reshape(6, 6)[1:5, 1:4])
    assert np.array_equal(only, _gather(ctx, grid, tile, rect, dtype, fill, idx[[4, 2]], tiles[[4, 2]], status=st[[4, 2]]))
    # nothing listed, and nothing listed for the rectangle: all fill
    assert (_gather(ctx, grid, tile, whole, dtype, fill, np.zeros(0, np.int32), np.zeros((0, cells), dtype)) == fill).all()
    assert (_gather(ctx, grid, tile, rect, dtype, fill, idx[[0, 1, 2]], tiles[[0, 1, 2]]) == fill).all()
    # the cut: an index outside the grid's tiles is GF_ERR_BOUNDS and its tile's memory stays as it was
    block = rng.integers(-30000, 30000, (10, 10)).astype(dtype)
    listed = np.array([2, 4, 0, -1, 3, 1, 2**31 - 1], np.int32)
    bad = (listed < 0) | (listed >= 4)
    for before in (None, np.full((listed.size, cells), 1234, dtype)):
        cut, cst = _cut(ctx, grid, tile, whole, dtype, fill, block, listed, before=before)
        assert cst.tolist() == [0, -2, 0, -2, 0, 0, -2]
        assert (cut[bad] == (_sentinel(dtype) if before is None else 1234)).all()
        good = np.flatnonzero(~bad)
        want = B.tiles_from_block(grid, tile, whole, block, listed[good], fill, before=None if before is None else before[good])
        assert np.array_equal(cut[good], want)


# ---------------------------------------------------------------- 4. records -> blocks

TILE4, GRID4 = (40, 60), (100, 200)
FILLS4 = [-123, None, np.float32(-7.5)]             # (the int-coded-float element is filled with its own fill_f, a NaN)


@pytest.fixture(scope="module")
def records4(ctx, master5):
    """tile records of three elements (short, ICF, float) for the 3 x 4 tiles of a 100 x 200 grid in shuffled order, packed and
    standard-form elements mixed; tile 5 twice; one record of a tile index beyond the grid; tile 3's only record and the later one
    of tile 2 with a flipped bit (the checksum notices), a second record of tile 11 truncated to 24 bytes.  With what
    gf_tile_record_decode_batch_elems_dev says about the same bytes."""
    import gridfour_amd
    nr, nc = TILE4
    enc = gridfour_amd.CodecMasterHip(context=ctx)
    flt = gridfour_amd.CodecFloatHip(context=ctx, level=6)
    src = [a[:16] for a in RE._three_sources(nr, nc)]
    cells = nr * nc
    std_size = [(2 * cells + 3) & ~3, 4 * cells, 4 * cells]
    packs = [enc.encode_batch(nr, nc, src[0])[0], enc.encode_batch(nr, nc, src[1])[0], flt.encode_floats_batch(2, nr, nc, src[2])]
    std = [np.where(src[0] == NULL, -32768, src[0]).astype("<i2"), src[1].astype("<i4"), src[2].astype("<f4")]
    index_of = [7, 2, 11, 5, 0, 9, 3, 12, 5, 1, 10, 6, 4, 8, 2, 11]      # record -> tile
    records, forms = [], set()
    for i, idx in enumerate(index_of):
        els = []
        for e in range(3):
            pk = packs[e][i]
            if (i >> e) & 1 and pk is not None and len(pk) != std_size[e]:
                els.append(pk)
                forms.add((e, "packed"))
            else:
                els.append(std[e][i].tobytes() + b"\0" * (std_size[e] - std[e][i].nbytes))
                forms.add((e, "standard"))
        records.append(_frame_elems(idx, els))
    assert len(forms) == 6
    records[6] = _flip(records[6], 40, 2)
    records[14] = _flip(records[14], 33, 6)
    records[15] = records[15][:24]
    blob, offsets = _shifted(records, seed=4)
    idx, vals, st = master5.record_blob_elems_dev(nr, nc, blob, offsets, RE.ELEMS3, verify_checksums=True)
    assert (st[:, [6, 14, 15]] != 0).all() and (np.delete(st, [6, 14, 15], axis=1) == 0).all(), st.tolist()
    assert idx[6] == 3 and idx[14] == 2 and idx[15] == -1                  # (a record whose head fails names no tile)
    return dict(blob=blob, offsets=offsets, idx=idx, vals=vals, st=st)


def _model4(r, rect):
    """per element the block's bits: the model over the good tiles of the elements call, fill elsewhere"""
    want = []
    for e, f in enumerate(FILLS4):
        v = _bits(r["vals"][e])
        fill = np.asarray(RE.ICF3[4] if f is None else f, r["vals"][e].dtype).reshape(1).view(v.dtype)[0]
        want.append(B.block_from_tiles(GRID4, TILE4, rect, r["idx"], v, fill, ok=r["st"][e] == 0))
    return want


def _read4(master, r, rect, host=False):
    read = master.read_block if host else master.read_block_dev
    return read(TILE4[0], TILE4[1], GRID4, rect, r["blob"], r["offsets"], RE.ELEMS3, fills=FILLS4, verify_checksums=True)


def test_records_to_blocks(master5, records4):
    r = records4
    whole, small = (0, 0) + GRID4, (13, 27, 80, 150)
    for rect in (whole, small, whole):                                    # (the smaller block between two whole ones: no stale cells)
        blocks, st = _read4(master5, r, rect)
        assert np.array_equal(st, r["st"]), (st.tolist(), r["st"].tolist())
        for e, want in enumerate(_model4(r, rect)):
            assert blocks[e].dtype == r["vals"][e].dtype
            assert np.array_equal(_bits(blocks[e]), want), (rect, e)
    # what the batch covered: tile 3 and tile 2 (its later record failed) read as fill, the later record of tile 5 counts, the
    # truncated record hides nothing of tile 11, tile 12 is nowhere
    assert (blocks[0][:40, 120:] == -123).all() and np.isnan(blocks[1][:40, 120:]).all() and (blocks[2][:40, 120:] == np.float32(-7.5)).all()
    assert np.array_equal(blocks[0][40:80, 60:120], r["vals"][0][8].reshape(40, 60))
    assert not np.array_equal(r["vals"][0][8], r["vals"][0][3])
    assert np.array_equal(blocks[0][80:, 180:], r["vals"][0][2].reshape(40, 60)[:20, :20])


def test_host_form_equals_the_device_form(master5, records4):
    for rect in ((0, 0) + GRID4, (99, 1, 1, 199)):
        hb, hs = _read4(master5, records4, rect, host=True)
        db, ds = _read4(master5, records4, rect)
        assert np.array_equal(hs, ds)
        for h, d in zip(hb, db):
            assert h.dtype == d.dtype and np.array_equal(_bits(h), _bits(d))


def test_no_records_is_all_fill(master5):
    rect = (5, 6, 50, 70)
    for host in (False, True):
        read = master5.read_block if host else master5.read_block_dev
        blocks, st = read(TILE4[0], TILE4[1], GRID4, rect, np.zeros(16, np.uint8), np.zeros(1, np.uint64), RE.ELEMS3, fills=FILLS4)
        assert st.shape == (3, 0)
        assert (blocks[0] == -123).all() and np.isnan(blocks[1]).all() and (blocks[2] == np.float32(-7.5)).all()


# ---------------------------------------------------------------- 5. two threads on one context; the gather in a hipGraph

def test_block_read_beside_a_decode_from_another_thread(master5, records4):
    r = records4
    rect = (13, 27, 80, 150)
    want = _model4(r, rect)
    errors = []
    start = threading.Barrier(2)

    def blocks(rounds):
        try:
            start.wait()
            for k in range(rounds):
                got, st = _read4(master5, r, rect)
                if not (np.array_equal(st, r["st"]) and all(np.array_equal(_bits(g), w) for g, w in zip(got, want))):
                    errors.append(("block", k))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def tiles(rounds):
        try:
            start.wait()
            for k in range(rounds):
                idx, vals, st = master5.record_blob_elems_dev(TILE4[0], TILE4[1], r["blob"], r["offsets"], RE.ELEMS3, verify_checksums=True)
                ok = st == 0
                if not (np.array_equal(st, r["st"]) and all(np.array_equal(_bits(v)[ok[e]], _bits(r["vals"][e])[ok[e]]) for e, v in enumerate(vals))):
                    errors.append(("tiles", k))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=blocks, args=(4,)), threading.Thread(target=tiles, args=(4,))]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert not any(t.is_alive() for t in th), "a thread hangs on the context's lock"
    assert not errors, errors[:3]


def test_gather_replayed_from_a_graph():
    import gridfour_amd
    hip = TG._hip()
    ctx = gridfour_amd.GvrsHipContext(0)
    tile, grid, rect = (7, 9), (23, 31), (2, 3, 20, 27)
    nrt, nct = B.tiles_of(grid, tile)
    nt, fill = nrt * nct, 0x80000000
    rng = np.random.default_rng(8)
    order = rng.permutation(nt)
    bufs = []
    graph, gexec = C.c_void_p(), C.c_void_p()
    try:
        d_tiles = Guarded(ctx, nt * 63, np.uint32)
        bufs.append(d_tiles)
        d_block = Guarded(ctx, rect[2] * rect[3], np.uint32)
        bufs.append(d_block)
        d_idx = _i32(ctx, order)
        bufs.append(d_idx)
        call = lambda: ctx.block_from_tiles_dev(grid + tile, rect, INT, fill, nt, d_idx.ptr, d_tiles.ptr, d_block.ptr)
        call()                                       # outside the capture: the module is loaded, the slot table has its size
        ctx.synchronize()
        stream = C.c_void_p(ctx.stream)
        assert hip.hipStreamBeginCapture(stream, 0) == 0               # hipStreamCaptureModeGlobal
        try:
            call()
        finally:
            ended = hip.hipStreamEndCapture(stream, C.byref(graph))
        assert ended == 0 and graph.value
        assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
        for k in range(2):
            tiles = rng.integers(0, 2**32 - 1, (nt, 63)).astype(np.uint32)
            d_tiles.put(tiles)
            d_block.put(np.zeros(rect[2] * rect[3], np.uint32))
            ctx.synchronize()
            assert hip.hipGraphLaunch(gexec, stream) == 0
            ctx.synchronize()
            assert np.array_equal(d_block.get().reshape(rect[2], rect[3]), B.block_from_tiles(grid, tile, rect, order, tiles, fill)), k
    finally:
        if gexec.value:
            hip.hipGraphExecDestroy(gexec)
        if graph.value:
            hip.hipGraphDestroy(graph)
        for b in bufs:
            b.free()
        ctx.close()
