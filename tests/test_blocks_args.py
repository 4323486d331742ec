"""CPU-only: gf_block_from_tiles_dev, gf_tiles_from_block_dev, gf_block_read_elems_dev and gf_block_read_elems reject what the host
can check with GF_ERR_ARG / GF_ERR_UNSUPPORTED before the context or a device is looked at; a rectangle that touches the grid's last
row and column is accepted, one cell beyond is not; without a device valid arguments fail as the other _dev entry points do."""
import ctypes as C

import numpy as np

from gridfour_amd import _lib
from gridfour_amd.codec import _ELEM_SPEC

STD = np.array([1, 2, 0, 3], np.int32)          # the standard codec list (include/gvrs_hip_codec.h)
INT, SHORT, FLOAT, ICF = 0, 1, 2, 3
GRID = (10, 12, 4, 5)                           # rows, columns of the grid; rows, columns of a tile
RECT = (2, 3, 6, 7)                             # row0, col0, rows, columns
FORMS = ("gather", "cut", "read_dev", "read")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _specs(*types, scale=1.0, fill_i=0):
    s = np.zeros(len(types), _ELEM_SPEC)
    s["type"] = types
    s["scale"] = scale
    s["fill_i"] = fill_i
    return s


def _buffers():
    # host memory standing in for device memory, and for a context: the argument checks must come before either is touched
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blob=np.zeros(256, np.uint8), off=np.array([0, 64, 128], np.uint64),
                idx=np.zeros(2, np.int32), val=np.zeros((16, 256), np.int32), blk=np.zeros(256, np.int32), st=np.zeros(16 * 2, np.int32))


def _call(L, b, form, ctx="ctx", grid=GRID, rect=RECT, elem_type=INT, n=2, idx="idx", tiles="val", block="blk", st="st", codecs=STD,
          n_codecs=4, specs=None, n_elems=None, blob="blob", off="off", blocks="val", null_block=None, blob_shift=0):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    ga, ra = np.array(GRID if grid is None else grid, np.int32), np.array(RECT if rect is None else rect, np.int32)    # (alive during the call)
    pg = None if grid is None else _p(ga)
    pr = None if rect is None else _p(ra)
    if form == "gather":
        return L.gf_block_from_tiles_dev(g(ctx), None, pg, pr, elem_type, 0, n, g(idx), g(st), g(tiles), g(block))
    if form == "cut":
        return L.gf_tiles_from_block_dev(g(ctx), None, pg, pr, elem_type, 0, 0, g(block), n, g(idx), g(tiles), g(st))
    specs = _specs(INT, FLOAT) if specs is None else specs
    n_elems = len(specs) if n_elems is None and specs is not False else n_elems
    ptrs = (C.c_void_p * 17)(*[b["val"][e % 16].ctypes.data for e in range(17)])
    if null_block is not None:
        ptrs[null_block] = None
    pv = None if blocks is None else ptrs
    ps = None if specs is False else _p(specs)
    pc = None if codecs is None else _p(codecs)
    pb = g(blob)
    if pb is not None and blob_shift:
        pb = C.c_void_p(pb.value + blob_shift)
    if form == "read_dev":
        return L.gf_block_read_elems_dev(g(ctx), None, pc, n_codecs, ps, n_elems, pg, pr, n, pb, b["blob"].size, g(off), 1, pv, g(st))
    return L.gf_block_read_elems(g(ctx), pc, n_codecs, ps, n_elems, pg, pr, n, pb, g(off), 1, pv, g(st))


def _untouched(b):
    assert (b["st"] == 0).all() and (b["val"] == 0).all() and (b["idx"] == 0).all() and (b["blk"] == 0).all()


def test_geometry_is_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in FORMS:
        for i in range(4):                                             # each of the eight numbers below its least value
            for v in (0, -1, -2**31):
                grid = list(GRID)
                grid[i] = v
                assert _call(L, b, form, grid=grid) == _lib.ERR_ARG, (form, "grid", i, v)
                rect = list(RECT)
                rect[i] = v if i >= 2 else min(v, -1)
                assert _call(L, b, form, rect=rect) == _lib.ERR_ARG, (form, "rect", i, v)
        assert _call(L, b, form, grid=None) == _lib.ERR_ARG
        assert _call(L, b, form, rect=None) == _lib.ERR_ARG
        # not wholly inside the grid: one cell beyond its last row, its last column; far beyond (no 32-bit wrap-around)
        assert _call(L, b, form, rect=(4, 3, 7, 7)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(2, 5, 6, 8)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(10, 0, 1, 1)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(0, 12, 1, 1)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(2**31 - 1, 0, 2**31 - 1, 1)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(0, 2**31 - 1, 1, 2**31 - 1)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(0, 0, 11, 12)) == _lib.ERR_ARG
        assert _call(L, b, form, rect=(0, 0, 10, 13)) == _lib.ERR_ARG
    _untouched(b)


def test_pointers_and_elements_are_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in ("gather", "cut"):
        for null in ("ctx", "idx", "tiles", "block"):
            assert _call(L, b, form, **{null: None}) == _lib.ERR_ARG, (form, null)
        for t in (-1, 4, 99):
            assert _call(L, b, form, elem_type=t) == _lib.ERR_ARG, (form, t)
    nine = np.array([1, 9, 0, 3], np.int32)
    for form in ("read_dev", "read"):
        for null in ("ctx", "blob", "off", "st"):
            assert _call(L, b, form, **{null: None}) == _lib.ERR_ARG, (form, null)
        assert _call(L, b, form, blocks=None) == _lib.ERR_ARG
        assert _call(L, b, form, null_block=1) == _lib.ERR_ARG                       # one of the n_elems block pointers
        assert _call(L, b, form, specs=False, n_elems=2) == _lib.ERR_ARG
        assert _call(L, b, form, codecs=None) == _lib.ERR_ARG
        assert _call(L, b, form, n_elems=0) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(*([INT] * 17))) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(INT, 4)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(ICF, scale=0.0)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(ICF, FLOAT, scale=np.nan)) == _lib.ERR_ARG
        assert _call(L, b, form, codecs=nine) == _lib.ERR_ARG
        assert _call(L, b, form, codecs=np.ones(256, np.int32), n_codecs=256) == _lib.ERR_ARG
        # the fill value of a SHORT element must be an int16; an INT's may be anything
        assert _call(L, b, form, specs=_specs(SHORT, fill_i=32768)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(INT, SHORT, fill_i=-32769)) == _lib.ERR_ARG
    for shift in (1, 2, 3):
        assert _call(L, b, "read_dev", blob_shift=shift) == _lib.ERR_ARG             # an unaligned d_blob
    _untouched(b)


def test_limits_are_unsupported():
    """more than 0x7fffffff tiles in the grid (46,341 x 46,341 tiles of one cell), in a list, or instances; the argument checks
    come first.  Nothing is read."""
    L = _lib.lib()
    b = _buffers()
    big = (46341, 46341, 1, 1)
    for form in FORMS:
        assert _call(L, b, form, grid=big, rect=(0, 0, 1, 1)) == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, grid=big, rect=(46341, 0, 1, 1)) == _lib.ERR_ARG, form
        assert _call(L, b, form, grid=(2**15, 2**13, 2**15, 2**13), rect=(0, 0, 1, 1)) == _lib.ERR_UNSUPPORTED, form   # 2^28 cells in a tile
    for form in ("gather", "cut"):
        assert _call(L, b, form, n=2**31) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, form, n=2**31, elem_type=7) == _lib.ERR_ARG
    for form in ("read_dev", "read"):
        assert _call(L, b, form, specs=_specs(INT), n=2**31) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, form, specs=_specs(INT, FLOAT), n=2**30) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, form, specs=_specs(INT), n=2**31, rect=(0, 0, 11, 1)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(SHORT, fill_i=40000), n=2**31) == _lib.ERR_ARG
    _untouched(b)


def test_valid_arguments_need_a_device():
    """rectangles that touch the grid's last row and column pass the checks: with a device they run, without one they fail as
    another _dev entry point does on the same stand-in context (there is no CPU path behind them)"""
    L = _lib.lib()
    b = _buffers()
    assert _call(L, b, "cut", n=0) == _lib.OK                                          # nothing to cut
    if L.gf_device_count() > 0:
        return
    lens = np.array([64, 64], np.uint32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), b["blob"].size, _p(b["off"]), 0, _p(lens),
                                             _p(b["val"]), _p(b["st"]))
    assert want < 0
    for form in FORMS:
        for rect in (RECT, (0, 0, 10, 12), (9, 11, 1, 1), (4, 7, 6, 5)):
            assert _call(L, b, form, rect=rect) == want, (form, rect)
        for n in (0,) if form != "cut" else ():                                        # an all-fill block needs a device too
            assert _call(L, b, form, n=n) == want, form
    _untouched(b)
