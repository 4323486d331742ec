"""CPU-only: the numpy model of a block write (tests/block_write_ref.py) against answers worked out by hand from
TileElementIntCodedFloat.setValue (TileElementIntCodedFloat.java:152-169), the default ranges of the element specifications and
TileElement*.hasValidData.  The GPU tests compare the library with this model, so the model is pinned here first."""
import numpy as np

import block_write_ref as W

F32 = np.float32
INT_MIN, INT_MAX = -2**31, 2**31 - 1
NAN = F32(np.nan)


def _icf(scale=1.0, offset=0.0, fill_i=INT_MIN, fill_f=NAN):
    return ("icf", scale, offset, fill_i, fill_f)


def _one(v, el, rng=None):
    code, bad = W.icf_convert(np.array([v], F32), el, rng)
    return int(code[0]), bool(bad[0])


def test_icf_rounding_is_floor_of_x_plus_half():
    assert _one(1.25, _icf(10.0)) == (13, False)                  # 12.5 + 0.5 = 13.0
    assert _one(-1.25, _icf(10.0)) == (-12, False)                # -12.5 + 0.5 = -12.0: not round-half-away
    assert _one(0.04, _icf(10.0)) == (0, False)
    assert _one(-0.06, _icf(10.0)) == (-1, False)
    assert _one(7.0, _icf(2.0, 3.0)) == (8, False)                # (7 - 3) * 2


def test_icf_default_range_and_saturation():
    lo, hi = W.default_range(_icf())
    assert lo == F32(-2147483648.0) and hi == F32(2147483648.0)   # (float)(INT_MIN + 1), (float)(INT_MAX - 1): both round outwards
    assert _one(F32(2147483648.0), _icf(fill_i=5)) == (INT_MAX, False)           # passes the range check, the cast saturates
    assert _one(F32(-2147483648.0), _icf(fill_i=5)) == (INT_MIN, False)
    nxt = np.nextafter(F32(2147483648.0), F32(np.inf))
    assert _one(nxt, _icf(fill_i=5)) == (5, True)                 # one float beyond: out of range
    assert _one(F32(np.inf), _icf(fill_i=5)) == (5, True)
    # scale 10, offset 1: the bounds are computed in float32, each operation rounded once
    lo, hi = W.default_range(_icf(10.0, 1.0))
    assert lo == F32(F32(INT_MIN + 1) / F32(10.0)) + F32(1.0) and hi == F32(F32(INT_MAX - 1) / F32(10.0)) + F32(1.0)


def test_icf_fill_is_float_equals():
    payload = np.array([0x7fc00001, 0xffc12345, 0x7f800001], np.uint32).view(F32)          # NaNs of any payload
    code, bad = W.icf_convert(payload, _icf(fill_i=-7, fill_f=NAN))
    assert (code == -7).all() and not bad.any()
    code, bad = W.icf_convert(payload, _icf(fill_i=-7, fill_f=F32(-9999.0)))               # a NaN and a non-NaN fill: out of range
    assert bad.all()
    assert _one(F32(-9999.0), _icf(fill_i=-7, fill_f=F32(-9999.0))) == (-7, False)
    # -0.0 is not the fill +0.0 by Float.equals: it is converted, to code 0
    assert _one(F32(-0.0), _icf(fill_i=-7, fill_f=F32(0.0))) == (0, False)
    assert _one(F32(0.0), _icf(fill_i=-7, fill_f=F32(0.0))) == (-7, False)
    # the fill passes even where it lies outside the range
    assert _one(F32(-9999.0), _icf(fill_i=-7, fill_f=F32(-9999.0)), rng=(0.0, 1.0)) == (-7, False)
    assert _one(F32(2.0), _icf(fill_i=-7, fill_f=F32(-9999.0)), rng=(0.0, 1.0)) == (-7, True)


def test_integer_ranges():
    v, bad = W.set_values(np.array([INT_MIN, INT_MIN + 1, 0, INT_MAX], np.int32), "int", fill=7)
    assert list(bad) == [True, False, False, False]                # default [INT_MIN + 1, INT_MAX]
    v, bad = W.set_values(np.array([INT_MIN, 5], np.int32), "int")  # the default fill is INT_MIN: the fill always passes
    assert not bad.any()
    v, bad = W.set_values(np.array([-32768, -32767, 32767, 100], np.int16), "short", fill=100, rng=(-5, 5))
    assert list(bad) == [True, True, True, False]
    v, bad = W.set_values(np.array([-32768, -32767, 32767], np.int16), "short")
    assert not bad.any()                                           # -32768 is the default fill
    v, bad = W.set_values(np.array([-32768, -32767, 32767], np.int16), "short", fill=0)
    assert list(bad) == [True, False, False]


def test_float_ranges_and_valid_data():
    cells = np.array([0.0, -0.0, 1.5, np.inf, -np.inf, np.nan], F32)
    v, bad = W.set_values(cells, "float", fill=0.0)
    assert list(bad) == [False, False, False, False, False, True]   # a NaN with a non-NaN fill is out of range
    assert v.view(np.uint32)[1] == 0x80000000                       # cells move as bits
    v, bad = W.set_values(cells, "float")                           # NaN fill: any NaN is the fill
    assert not bad.any()
    v, bad = W.set_values(cells, "float", fill=0.0, rng=(1.0, 2.0))
    assert list(bad) == [False, True, False, True, True, True]      # +0.0 is the fill; -0.0 is not (Float.equals) and is < 1
    # hasValidData: with a 0.0 fill a -0.0 cell is NOT valid data (the float comparison), with a NaN fill everything but a NaN is
    assert list(W.valid_mask(np.array([0.0, -0.0, 1e-45], F32), "float", 0.0)) == [False, False, True]
    assert list(W.valid_mask(np.array([np.nan, 0.0, -0.0], F32), "float")) == [False, True, True]
    assert list(W.valid_mask(np.array([3, 4], np.int32), "int", 3)) == [False, True]
    assert list(W.valid_mask(np.array([-7, 0], np.int32), _icf(fill_i=-7))) == [False, True]


def test_cut_statuses_and_precedence():
    grid, tile = (6, 6), (3, 3)
    blk = np.arange(36, dtype=np.int32).reshape(6, 6) + 1
    idx, tiles, pre = W.cut(grid, tile, (0, 0, 6, 6), [blk], ["int"], fills=[0])
    assert list(idx) == [0, 1, 2, 3] and (pre == 0).all()
    assert list(tiles[0][1]) == [4, 5, 6, 10, 11, 12, 16, 17, 18]
    # tile 1 all fill -> DECLINED; one cell out of range in tile 2 -> ERR_BOUNDS; tile 3 both (BOUNDS wins over nothing else valid)
    b = blk.copy()
    b[0:3, 3:6] = 0
    b[4, 1] = 1000
    idx, tiles, pre = W.cut(grid, tile, (0, 0, 6, 6), [b], ["int"], fills=[0], ranges=[(0, 100)])
    assert list(pre) == [0, W.DECLINED, W.ERR_BOUNDS, 0]
    # a partly covered tile: fill outside without an old tile, the old cells with one; an unreadable old record comes first
    idx, tiles, pre = W.cut(grid, tile, (1, 1, 1, 1), [np.array([[1000]], np.int32)], ["int"], fills=[0], ranges=[(0, 100)],
                            before={0: [np.full(9, 9, np.int32)]})
    assert list(idx) == [0] and list(pre) == [W.ERR_BOUNDS] and list(tiles[0][0]) == [9, 9, 9, 9, 1000, 9, 9, 9, 9]
    idx, tiles, pre = W.cut(grid, tile, (1, 1, 1, 1), [np.array([[1000]], np.int32)], ["int"], fills=[0], ranges=[(0, 100)], before={0: -1})
    assert list(pre) == [-1]
    idx, tiles, pre = W.cut(grid, tile, (1, 1, 1, 1), [np.array([[0]], np.int32)], ["int"], fills=[0])
    assert list(pre) == [W.DECLINED] and (tiles[0] == 0).all()
    idx, tiles, pre = W.cut(grid, tile, (1, 1, 1, 1), [np.array([[0]], np.int32)], ["int"], fills=[0], before={0: [np.full(9, 9, np.int32)]})
    assert list(pre) == [0]                                         # the kept old cells are data
    # a wholly covered tile ignores its old record, readable or not
    idx, tiles, pre = W.cut(grid, tile, (0, 0, 3, 3), [blk[:3, :3]], ["int"], fills=[0], before={0: -1})
    assert list(pre) == [0]
    assert W.tile_rect((37, 53), (8, 10), (32, 50, 5, 3)) == (4, 5, 1, 1)
    assert W.tile_rect((37, 53), (8, 10), (7, 9, 2, 2)) == (0, 0, 2, 2)


def test_expected_lays_out_zero_length_records():
    def encode(indices, tiles):
        return [b"r%d" % i for i in indices], np.zeros((1, len(indices)), np.uint8), np.zeros(len(indices), np.int32)
    b = np.ones((6, 6), np.int32)
    b[0:3, 3:6] = 0
    idx, recs, off, used, st = W.expected(encode, (6, 6), (3, 3), (0, 0, 6, 6), [b], ["int"], fills=[0])
    assert recs == [b"r0", b"", b"r2", b"r3"] and list(off) == [0, 2, 2, 4, 6]
    assert list(used[0]) == [0, 255, 0, 0] and list(st) == [0, 1, 0, 0]
