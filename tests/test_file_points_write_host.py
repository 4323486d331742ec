"""Writes at scattered points, as far as no device is needed: the three entry points exist in the library and in _lib.py with the
header's signatures; every GF_ERR_ARG / GF_ERR_UNSUPPORTED case is answered before the context or a device is looked at (a
context that is no context is never touched); gf_file_update_plan_tiles equals gf_file_update_plan on a rectangle of as many
tiles; and the model file_points_write_ref.py is checked against itself: a point set that changes nothing but rewrites its tiles
gives the image that gvrs_file_update_ref gives for those tiles' own re-encoded records."""
import ctypes as C
import os
import re

import numpy as np

import gridfour_amd
from gridfour_amd import _lib
from gridfour_amd.codec import _ptr

import file_points_write_ref as M
import file_update_cases as U
import gvrs_file_build as B
import gvrs_file_update_ref as R

OK, ERR_ARG, ERR_UNSUPPORTED = _lib.OK, _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
NAMES = ("gf_file_update_plan_tiles", "gf_file_update_points_elems_dev", "gf_file_update_points_elems")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (19, 22, 5, 7)                                             # 4 x 4 tiles of 5 x 7 cells, the last row and column cut by the grid


def test_the_entry_points_exist_with_the_headers_signatures():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "gvrs_hip_codec.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and getattr(L, name).argtypes == argtypes
        decl = re.search(r"gf_status %s\((.*?)\);" % name, header, re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(argtypes), (name, params)
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a in (C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)), (name, p)
            elif p.startswith("size_t"):
                assert a is C.c_size_t, (name, p)
            elif p.startswith("int64_t"):
                assert a is C.c_int64, (name, p)
            else:
                assert p.startswith("int ") and a is C.c_int, (name, p)
    for method in ("update_points", "update_points_host", "update_plan_tiles"):
        assert callable(getattr(gridfour_amd.GvrsFileHip, method))


def image_of(codec_ids=(), grid=GRID, dir_rect=None, elements=None):
    elements = [B.element("z", "int", fill=-9999), B.element("s", "short", fill=-1)] if elements is None else elements
    n_cells = grid[2] * grid[3]
    records = {} if dir_rect is not None else {t: B.standard_record(t, [np.arange(n_cells, dtype=np.int32) + 100 * t, np.full(n_cells, t, np.int16)])
                                                for t in (0, 1, 5, 6, 15)}
    return B.build_image(grid, elements, records, codec_ids, dir_rect=dir_rect)[0]


def test_plan_tiles_equals_the_plan_of_a_rectangle():
    f = gridfour_amd.GvrsFileHip(image_of(("GvrsHuffman",)))
    u = f.update_begin()
    for rect, n in (((0, 0, 5, 7), 1), ((0, 0, 5, 8), 2), ((4, 6, 7, 9), 9), ((0, 0, 19, 22), 16), (None, 16)):
        assert f.update_plan_tiles(u, n) == u.plan(rect)
    assert f.update_plan_tiles(u, 0)[1] == len(u.free_list) + 3
    most, cap = C.c_uint64(), C.c_uint64()
    L = _lib.lib()
    assert L.gf_file_update_plan_tiles(None, 1, C.byref(most), C.byref(cap)) == ERR_ARG
    assert L.gf_file_update_plan_tiles(u.handle, 17, C.byref(most), C.byref(cap)) == ERR_ARG        # more tiles than the grid has
    assert L.gf_file_update_plan_tiles(u.handle, 3, None, None) == OK


def call(L, name, ctx, u, n, rows, cols, values, max_tiles, image, cap, outs, touched):
    """either form with its outputs in host arrays (nothing is written by a refused call)"""
    need, fst, pst, idx, st = outs
    if name.endswith("_dev"):
        return L.gf_file_update_points_elems_dev(ctx, u, n, rows, cols, values, max_tiles, 0, U.TIME, image, cap, need, fst, pst, idx, st, None, touched)
    return L.gf_file_update_points_elems(ctx, u, n, rows, cols, values, max_tiles, 0, U.TIME, image, cap, C.cast(need, C.POINTER(C.c_uint64)), pst, idx,
                                         st, None, touched)


def test_the_writes_refuse_their_arguments_before_a_context_is_looked_at():
    L = _lib.lib()
    no_context = np.full(4096, 0x5A, np.uint8)                    # not a context: a refusal must not read it
    ctx = _ptr(no_context)
    rows, cols = np.zeros(2, np.int32), np.zeros(2, np.int32)
    z, s = np.zeros(2, np.int32), np.zeros(2, np.int16)
    need, fst = np.zeros(2, np.uint64), np.zeros(2, np.int32)
    pst, idx, st = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    outs = (_ptr(need), _ptr(fst), _ptr(pst), _ptr(idx), _ptr(st))
    n = C.c_size_t()
    touched = C.byref(n)

    def handle(image):
        f = gridfour_amd.GvrsFileHip(image)
        return f, f.update_begin()

    for name in NAMES[1:]:
        f, u = handle(image_of(("GvrsHuffman",)))
        room = np.zeros(u.plan()[0] + 64, np.uint8)
        room[:f.image.size] = f.image
        before = room.copy()
        image, cap = _ptr(room), room.size - 64
        values = (C.c_void_p * 2)(z.ctypes.data, s.ctypes.data)
        good = (ctx, u.handle, 2, _ptr(rows), _ptr(cols), values, 4, image, cap, outs, touched)
        for k in (0, 1, 3, 4, 5, 7, 10):                           # a null pointer in each place
            args = list(good)
            args[k] = None
            assert call(L, name, *args) == ERR_ARG, (name, k)
        for k in range(5):                                         # ... and in each output (the host form has no file status)
            o = list(outs)
            if name.endswith("_dev") or k != 1:
                o[k] = None
                assert call(L, name, *good[:9], tuple(o), touched) == ERR_ARG, (name, k)
        assert call(L, name, ctx, u.handle, 2, _ptr(rows), _ptr(cols), (C.c_void_p * 2)(z.ctypes.data, None), 4, image, cap, outs, touched) == ERR_ARG
        assert call(L, name, ctx, u.handle, 2, _ptr(rows), _ptr(cols), values, 4, image, f.image.size - 8, outs, touched) == ERR_ARG   # below the old size
        if name.endswith("_dev"):
            odd = C.c_void_p(room.ctypes.data + 4)
            assert call(L, name, ctx, u.handle, 2, _ptr(rows), _ptr(cols), values, 4, odd, cap, outs, touched) == ERR_ARG              # unaligned
        # counts beyond 0x7fffffff
        assert call(L, name, ctx, u.handle, 0x80000000, _ptr(rows), _ptr(cols), values, 4, image, cap, outs, touched) == ERR_UNSUPPORTED
        assert call(L, name, ctx, u.handle, 2, _ptr(rows), _ptr(cols), values, 0x40000000, image, cap, outs, touched) == ERR_UNSUPPORTED
        # a codec the library does not know
        f2, u2 = handle(image_of(("GvrsHuffman", "NoSuchCodec")))
        assert call(L, name, ctx, u2.handle, 2, _ptr(rows), _ptr(cols), values, 4, image, cap, outs, touched) == ERR_UNSUPPORTED
        # more than 2^27 tiles in the grid
        f3, u3 = handle(image_of(("GvrsHuffman",), grid=(16384, 8193, 1, 1), dir_rect=(0, 0, 1, 1)))
        assert call(L, name, ctx, u3.handle, 2, _ptr(rows), _ptr(cols), values, 4, image, cap, outs, touched) == ERR_UNSUPPORTED
        assert (room == before).all() and (no_context == 0x5A).all()
    # the device form takes only a list the device record writer takes: decided from the arguments alone
    f4, u4 = handle(image_of(B.STANDARD_IDS))
    room = np.zeros(u4.plan()[0], np.uint8)
    assert call(L, NAMES[1], ctx, u4.handle, 2, _ptr(rows), _ptr(cols), (C.c_void_p * 2)(z.ctypes.data, s.ctypes.data), 4, _ptr(room), room.size, outs,
                touched) == ERR_UNSUPPORTED
    # no points: GF_OK, nothing touched, nothing read -- not even the context
    f5, u5 = handle(image_of(("GvrsHuffman",)))
    room = np.zeros(u5.plan()[0], np.uint8)
    for name in NAMES[1:]:
        n.value = 77
        assert call(L, name, ctx, u5.handle, 0, None, None, (C.c_void_p * 2)(z.ctypes.data, s.ctypes.data), 0, _ptr(room), room.size, outs, touched) == OK
        assert n.value == 0 and not room.any()


def test_the_model_agrees_with_itself_on_a_rewrite_that_changes_nothing():
    """standard-form records, no library: every cell of tiles 1 and 6 and a few of tile 15 written with the values they hold"""
    image = image_of(())
    elems, fills = ["int", "short"], [-9999, -1]
    n_cells = GRID[2] * GRID[3]
    locate = M.directory_locate(image, GRID)
    old_tile = M.old_tile_reader(locate, image, M.standard_decode(elems, n_cells))
    rows, cols = [], []
    for t in (6, 1):
        tr, tc = divmod(t, 4)
        for k in range(n_cells):
            rows.append(tr * GRID[2] + k // GRID[3])
            cols.append(tc * GRID[3] + k % GRID[3])
    rows += [18, 15]                                              # tile 15, which the grid cuts: its cells beyond the edge stay
    cols += [21, 21]
    keep = [i for i in range(len(rows)) if rows[i] < GRID[0] and cols[i] < GRID[1]]
    rows, cols = np.array(rows, np.int32)[keep], np.array(cols, np.int32)[keep]
    values = [np.zeros(rows.size, np.int32), np.zeros(rows.size, np.int16)]
    for i, (r, c) in enumerate(zip(rows, cols)):
        t, at = M.cell_of(GRID, int(r), int(c))
        old = old_tile(t)
        values[0][i], values[1][i] = old[0][at], old[1][at]
    out, pst, tiles, tst, used = M.update(image, GRID, False, elems, fills, rows, cols, values, old_tile, M.standard_encode(True), U.TIME)
    assert tiles.tolist() == [1, 6, 15] and tst.tolist() == [0, 0, 0] and (pst == 0).all() and (used == 255).all()
    records = [bytes(image[p - 8:p - 8 + M.head_status(image, p)[1]]) for p in (locate(t)[1] for t in (1, 6, 15))]
    assert out == R.ref_update(image, 4, False, records, [1, 6, 15], U.TIME)[0]
    # ... and the sequence's rules on the same file: a later duplicate wins, a refused value leaves the earlier one, a point outside
    rows, cols = np.array([0, 0, 0, -1, 7], np.int32), np.array([8, 8, 8, 0, 15], np.int32)
    values = [np.array([5, 6, -2 ** 31, 1, 2], np.int32), np.array([7, -32768, 9, 1, -1], np.int16)]
    out, pst, tiles, tst, _ = M.update(image, GRID, False, elems, fills, rows, cols, values, old_tile, M.standard_encode(True), U.TIME)
    assert pst.tolist() == [[0, 0, M.ERR_BOUNDS, M.ERR_ARG, 0], [0, M.ERR_BOUNDS, 0, M.ERR_ARG, 0]]
    assert tiles.tolist() == [1, 6] and tst.tolist() == [0, 0]
    g = M.old_tile_reader(M.directory_locate(out, GRID), out, M.standard_decode(elems, n_cells))
    assert g(1)[0][1] == 6 and g(1)[1][1] == 9 and g(6)[0][2 * 7 + 1] == 2 and g(6)[1][2 * 7 + 1] == -1
