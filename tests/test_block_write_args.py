"""CPU-only: gf_block_tile_rect's numbers against the model, and what gf_block_write_elems_dev / gf_block_write_elems reject with
GF_ERR_ARG / GF_ERR_UNSUPPORTED before the context or a device is looked at: the geometry as the block reads, the record writer's and
(with old records) the record reader's argument checks, codec lists the device form cannot serve, and bad ranges."""
import ctypes as C

import numpy as np

import block_ref as B
import block_write_ref as W
from gridfour_amd import _lib
from gridfour_amd.codec import _ELEM_RANGE, _ELEM_SPEC

DEV = np.array([1, 3], np.int32)                # CodecHuffman, CodecCanonHuffman: a list the device form takes (gvrs_hip_codec.h)
STD = np.array([1, 2, 0, 3], np.int32)          # the standard list: CodecDeflate needs the host
INT, SHORT, FLOAT, ICF = 0, 1, 2, 3
GRID = (10, 12, 4, 5)
RECT = (2, 3, 6, 7)
FORMS = ("dev", "host")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _specs(*types, scale=1.0, fill_i=0):
    s = np.zeros(len(types), _ELEM_SPEC)
    s["type"] = types
    s["scale"] = scale
    s["fill_i"] = fill_i
    return s


def _ranges(*rows):
    r = np.zeros(len(rows), _ELEM_RANGE)
    for e, row in enumerate(rows):
        r[e] = row
    return r


def _buffers():
    fake = C.create_string_buffer(8192)
    return dict(ctx=C.cast(fake, C.c_void_p), keep=fake, blob=np.zeros(4096, np.uint8), off=np.zeros(64, np.uint64), idx=np.zeros(64, np.int32),
                val=np.zeros((16, 256), np.int32), st=np.zeros(64, np.int32), used=np.zeros(256, np.uint8), oblob=np.zeros(256, np.uint8),
                ooff=np.array([0, 64, 128], np.uint64))


def _call(L, b, form, ctx="ctx", grid=GRID, rect=RECT, codecs=DEV, n_codecs=None, specs=None, n_elems=None, ranges=None, blocks="val",
          null_block=None, n_old=0, oblob="oblob", ooff="ooff", blob="blob", cap=4096, off="off", idx="idx", used="used", st="st",
          blob_shift=0, oblob_shift=0):
    g = lambda k: None if k is None else (b[k] if k == "ctx" else _p(b[k]))
    ga, ra = np.array(GRID if grid is None else grid, np.int32), np.array(RECT if rect is None else rect, np.int32)
    pg, pr = (None if grid is None else _p(ga)), (None if rect is None else _p(ra))
    specs = _specs(INT, SHORT) if specs is None else specs
    n_elems = len(specs) if n_elems is None and specs is not False else n_elems
    n_codecs = (0 if codecs is None else len(codecs)) if n_codecs is None else n_codecs
    ptrs = (C.c_void_p * 17)(*[b["val"][e % 16].ctypes.data for e in range(17)])
    if null_block is not None:
        ptrs[null_block] = None
    pv = None if blocks is None else ptrs
    ps = None if specs is False else _p(specs)
    pc = None if codecs is None else _p(codecs)
    prg = None if ranges is None else _p(ranges)
    pb, pob = g(blob), g(oblob)
    if pb is not None and blob_shift:
        pb = C.c_void_p(pb.value + blob_shift)
    if pob is not None and oblob_shift:
        pob = C.c_void_p(pob.value + oblob_shift)
    if form == "dev":
        return L.gf_block_write_elems_dev(g(ctx), None, pc, n_codecs, ps, prg, n_elems, pg, pr, pv, n_old, pob, 128, g(ooff), 1, 1, pb, cap, g(off),
                                          g(idx), g(used), g(st))
    return L.gf_block_write_elems(g(ctx), pc, n_codecs, ps, prg, n_elems, pg, pr, pv, n_old, pob, g(ooff), 1, 1, pb, cap, g(off), g(idx), g(used),
                                  g(st))


def _untouched(b):
    for k in ("blob", "off", "idx", "val", "st", "used"):
        assert (b[k] == 0).all(), k


def test_tile_rect_matches_the_model():
    L = _lib.lib()
    cases = [((37, 53), (8, 10), (0, 0, 37, 53)), ((37, 53), (8, 10), (8, 10, 16, 20)), ((37, 53), (8, 10), (7, 9, 10, 12)),
             ((37, 53), (8, 10), (20, 31, 1, 1)),                    # a one-cell rectangle
             ((37, 53), (8, 10), (32, 0, 5, 53)),                    # the last, overhanging tile row
             ((37, 53), (8, 10), (36, 52, 1, 1)), ((70, 90), (32, 32), (31, 31, 34, 34)), ((70, 90), (32, 32), (0, 0, 70, 90)),
             ((5, 7), (5, 7), (0, 0, 5, 7)), ((1, 1), (1, 1), (0, 0, 1, 1))]
    for grid, tile, rect in cases:
        out = [C.c_int32(-1) for _ in range(4)]
        ga, ra = np.array(grid + tile, np.int32), np.array(rect, np.int32)
        assert L.gf_block_tile_rect(_p(ga), _p(ra), *[C.byref(x) for x in out]) == _lib.OK
        got = tuple(x.value for x in out)
        assert got == W.tile_rect(grid, tile, rect), (grid, tile, rect)
        nrt, nct = B.tiles_of(grid, tile)
        assert got[0] + got[2] <= nrt and got[1] + got[3] <= nct
    assert W.tile_rect((37, 53), (8, 10), (0, 0, 37, 53)) == (0, 0) + B.tiles_of((37, 53), (8, 10))


def test_tile_rect_rejects_what_the_geometry_check_rejects():
    L = _lib.lib()
    out = [C.c_int32(-1) for _ in range(4)]
    refs = [C.byref(x) for x in out]
    ga, ra = np.array(GRID, np.int32), np.array(RECT, np.int32)
    assert L.gf_block_tile_rect(None, _p(ra), *refs) == _lib.ERR_ARG
    assert L.gf_block_tile_rect(_p(ga), None, *refs) == _lib.ERR_ARG
    for k in range(4):
        args = list(refs)
        args[k] = None
        assert L.gf_block_tile_rect(_p(ga), _p(ra), *args) == _lib.ERR_ARG
    for rect in ((4, 3, 7, 7), (2, 5, 6, 8), (10, 0, 1, 1), (0, 12, 1, 1), (0, 0, 0, 1), (-1, 0, 1, 1), (2**31 - 1, 0, 2**31 - 1, 1)):
        rb = np.array(rect, np.int32)
        assert L.gf_block_tile_rect(_p(ga), _p(rb), *refs) == _lib.ERR_ARG, rect
    big, one = np.array((46341, 46341, 1, 1), np.int32), np.array((0, 0, 1, 1), np.int32)
    assert L.gf_block_tile_rect(_p(big), _p(one), *refs) == _lib.ERR_UNSUPPORTED
    cells = np.array((2**15, 2**13, 2**15, 2**13), np.int32)
    assert L.gf_block_tile_rect(_p(cells), _p(one), *refs) == _lib.ERR_UNSUPPORTED
    assert all(x.value == -1 for x in out)


def test_geometry_is_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    for form in FORMS:
        for i in range(4):
            for v in (0, -1, -2**31):
                grid = list(GRID)
                grid[i] = v
                assert _call(L, b, form, grid=grid) == _lib.ERR_ARG, (form, "grid", i, v)
                rect = list(RECT)
                rect[i] = v if i >= 2 else min(v, -1)
                assert _call(L, b, form, rect=rect) == _lib.ERR_ARG, (form, "rect", i, v)
        assert _call(L, b, form, grid=None) == _lib.ERR_ARG
        assert _call(L, b, form, rect=None) == _lib.ERR_ARG
        for rect in ((4, 3, 7, 7), (2, 5, 6, 8), (10, 0, 1, 1), (0, 12, 1, 1), (0, 0, 11, 12), (0, 0, 10, 13)):
            assert _call(L, b, form, rect=rect) == _lib.ERR_ARG, (form, rect)
        big = (46341, 46341, 1, 1)
        assert _call(L, b, form, grid=big, rect=(0, 0, 1, 1)) == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, grid=big, rect=(46341, 0, 1, 1)) == _lib.ERR_ARG, form
        assert _call(L, b, form, grid=(2**15, 2**13, 2**15, 2**13), rect=(0, 0, 1, 1)) == _lib.ERR_UNSUPPORTED, form
        assert _call(L, b, form, grid=big, rect=(0, 0, 1, 1), specs=_specs(INT, 9)) == _lib.ERR_ARG, form      # ARG before UNSUPPORTED
    _untouched(b)


def test_pointers_elements_and_lists_are_checked_before_the_device():
    L = _lib.lib()
    b = _buffers()
    nine = np.array([1, 9], np.int32)
    for form in FORMS:
        for null in ("ctx", "off", "idx", "st", "blob"):
            assert _call(L, b, form, **{null: None}) == _lib.ERR_ARG, (form, null)
        assert _call(L, b, form, blocks=None) == _lib.ERR_ARG
        assert _call(L, b, form, null_block=1) == _lib.ERR_ARG
        assert _call(L, b, form, specs=False, n_elems=2) == _lib.ERR_ARG
        assert _call(L, b, form, codecs=None, n_codecs=2) == _lib.ERR_ARG
        assert _call(L, b, form, n_elems=0) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(*([INT] * 17))) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(INT, 4)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(ICF, scale=0.0)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(ICF, INT, scale=np.nan)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(SHORT, fill_i=32768)) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(INT, SHORT, fill_i=-32769)) == _lib.ERR_ARG
        assert _call(L, b, form, codecs=nine) == _lib.ERR_ARG
        assert _call(L, b, form, codecs=np.ones(256, np.int32)) == _lib.ERR_ARG
        # old records: the reader's checks apply only when there are any (without any, null pointers pass: see
        # test_valid_arguments_need_a_device, the only place where a call that passes every check is made)
        assert _call(L, b, form, n_old=2, oblob=None) == _lib.ERR_ARG
        assert _call(L, b, form, n_old=2, ooff=None) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(INT), n_old=2**31) == _lib.ERR_UNSUPPORTED
        assert _call(L, b, form, specs=_specs(INT, FLOAT), codecs=np.array([1], np.int32), n_old=2**30) == _lib.ERR_UNSUPPORTED
    # the device form: alignment, and the lists of gf_tile_record_encode_batch_elems_dev
    for shift in (1, 2, 4):
        assert _call(L, b, "dev", blob_shift=shift) == _lib.ERR_ARG
    for shift in (1, 2, 3):
        assert _call(L, b, "dev", n_old=2, oblob_shift=shift) == _lib.ERR_ARG
    assert _call(L, b, "dev", codecs=STD) == _lib.ERR_UNSUPPORTED
    assert _call(L, b, "dev", codecs=np.array([1, 4], np.int32)) == _lib.ERR_UNSUPPORTED                      # LSOP12
    assert _call(L, b, "dev", codecs=np.array([1, 0], np.int32), specs=_specs(INT, FLOAT)) == _lib.ERR_UNSUPPORTED   # CodecFloat at work
    assert _call(L, b, "dev", codecs=STD, specs=_specs(INT, 7)) == _lib.ERR_ARG
    _untouched(b)


def test_bad_ranges_are_arg_errors():
    L = _lib.lib()
    b = _buffers()
    nan, inf = np.nan, np.inf
    for form in FORMS:
        assert _call(L, b, form, specs=_specs(INT), ranges=_ranges((5, 4, 0, 0))) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(INT, SHORT), ranges=_ranges((0, 9, 0, 0), (1, 0, 0, 0))) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(FLOAT), ranges=_ranges((0, 0, 1.0, 0.5))) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(FLOAT), ranges=_ranges((0, 0, nan, 1.0)), codecs=DEV) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(ICF), ranges=_ranges((0, 0, 0.0, nan))) == _lib.ERR_ARG
        assert _call(L, b, form, specs=_specs(ICF), ranges=_ranges((0, 0, inf, -inf))) == _lib.ERR_ARG
    _untouched(b)


def test_valid_arguments_need_a_device():
    """calls that pass every check are made only here, and only WITHOUT a device: the context is a stand-in and the "device" pointers
    are host memory, so nothing that passes the checks may reach a GPU.  Without one they fail as another _dev entry point does."""
    L = _lib.lib()
    b = _buffers()
    if L.gf_device_count() > 0:
        return
    lens = np.array([64, 64], np.uint32)
    want = L.gf_huffman_decode_batch_i32_dev(b["ctx"], None, 4, 4, 2, _p(b["blob"]), b["blob"].size, _p(b["oblob"]), 0, _p(lens), _p(b["val"]),
                                             _p(b["st"]))
    assert want < 0
    for form in FORMS:
        for rect in (RECT, (0, 0, 10, 12), (9, 11, 1, 1)):
            assert _call(L, b, form, rect=rect) == want, (form, rect)
        assert _call(L, b, form, n_old=2) == want, form
    assert _call(L, b, "host", codecs=STD) == want
    inf = np.inf
    for form in FORMS:
        # without old records their three arguments may be null
        assert _call(L, b, form, n_old=0, oblob=None, ooff=None) == want, form
        # the bounds that do not belong to the element's type are not looked at; min == max and infinite bounds are fine
        assert _call(L, b, form, specs=_specs(INT), ranges=_ranges((4, 4, 2.0, 1.0))) == want, form
        assert _call(L, b, form, specs=_specs(FLOAT), ranges=_ranges((9, 0, -inf, inf))) == want, form
        assert _call(L, b, form, specs=_specs(ICF), ranges=_ranges((9, 0, 1.0, 1.0))) == want, form
    _untouched(b)
