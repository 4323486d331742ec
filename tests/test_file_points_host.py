"""gf_file_cells_tiles / gf_file_interp_tiles (host arithmetic: no device, no context) held to the numpy restatement
file_points_ref.py over the reference's fifteen sample files and the grids of file_points_cases.py, the tiles_cap rules, and the
GF_ERR_ARG cases of the device and host forms of the reads at points with a NULL context: an error code, never a crash."""
import ctypes as C

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import _lib
from gridfour_amd.codec import _ptr

import file_points_cases as K
import file_points_ref as R
from test_file_open import FACTS, sample_path

OK, ERR_ARG = _lib.OK, _lib.ERR_ARG


def files(golden_dir):
    out = [gridfour_amd.GvrsFileHip(sample_path(golden_dir, k)) for k in range(15)]
    return out + [gridfour_amd.GvrsFileHip(K.image_of(g)) for g in K.EXTRA_GRIDS]


@pytest.fixture(scope="module")
def opened(golden_dir):
    return files(golden_dir)


def test_the_cases_cover_the_sample_grids():
    assert sorted({FACTS[k][0] for k in range(15)}) == sorted(K.SAMPLE_GRIDS)


def test_the_rank_chunk_constant_mirrors_the_kernels():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gridfour_amd", "csrc", "gvrs_kernels.h")).read()
    assert int(re.search(r"GF_POINTS_RANK_CHUNK = (\d+);", text).group(1)) == K.RANK_CHUNK_WORDS


def test_cells_tiles(opened):
    for f in opened:
        rows, cols = K.cell_points(f.grid)
        want = R.cells_touched(f.grid, rows, cols)
        got = f.cells_tiles(rows, cols)
        assert got.dtype == np.int32 and got.tolist() == want.tolist(), f.grid
        assert f.cells_tiles([-1, f.grid[0]], [0, 0]).size == 0                  # only cells outside the grid: nothing touched
        assert f.cells_tiles([], []).size == 0


@pytest.mark.parametrize("wrap", [0, 1, 2])
def test_interp_tiles(opened, wrap):
    some_wrapped = False
    for f in opened:
        rows, cols = K.window_points(f.grid)
        for k in range(len(K.FRINGES)):
            rf, cf = K.fringe_of(f.grid, k)
            spec = f.points_spec(0, wrap=wrap, row_fringe=rf, col_fringe=cf)
            ref = R.spec_of(f.grid, wrap, rf, cf)
            want = R.windows_touched(f.grid, ref, rows, cols)
            assert f.interp_tiles(spec, rows, cols).tolist() == want.tolist(), (f.grid, k)
            # one point at a time: its window's tiles alone, and none for a refused point
            per_point = R.window_tiles(f.grid, ref, rows, cols)
            for i in range(0, rows.size, 7):
                assert f.interp_tiles(spec, rows[i:i + 1], cols[i:i + 1]).tolist() == per_point[i], (f.grid, rows[i], cols[i])
            _, _, _, n1, _, _ = R.IR.window(ref, rows, cols)
            some_wrapped |= bool(((n1 < 4) & (n1 > 0)).any())
    assert some_wrapped == (wrap != 0)                                           # windows that take columns from both ends of the grid


def test_a_window_spans_three_tile_rows_and_sixteen_tiles(opened):
    f299, f11 = opened[15], opened[16]
    assert f299.grid == K.GRID299 and f11.grid == (5, 4, 1, 1)
    assert len(f299.interp_tiles(f299.points_spec(0), [2.0], [3.0])) == 6        # rows 1..4 and columns 2..5 of 2 x 3 tiles: 3 x 2 of them
    assert len(f11.interp_tiles(f11.points_spec(0), [2.0], [1.5])) == 16


def test_tiles_cap(opened):
    f = opened[15]
    rows, cols = K.cell_points(f.grid)
    want = R.cells_touched(f.grid, rows, cols)
    n = want.size
    assert n > 8
    L = _lib.lib()
    for cap in (0, 1, n - 1, n, n + 3):
        tiles = np.full(n + 4, -7, np.int32)
        count = C.c_size_t(99)
        st = L.gf_file_cells_tiles(f._h, rows.size, _ptr(rows), _ptr(cols), _ptr(tiles) if cap else None, cap, C.byref(count))
        assert st == OK and count.value == n
        assert tiles[:min(cap, n)].tolist() == want[:min(cap, n)].tolist() and (tiles[min(cap, n):] == -7).all()
    drows, dcols = K.window_points(f.grid)
    spec = f.points_spec(0, wrap=1)
    wantw = R.windows_touched(f.grid, R.spec_of(f.grid, 1), drows, dcols)
    for cap in (0, wantw.size - 1, wantw.size, wantw.size + 1):
        tiles = np.full(wantw.size + 4, -7, np.int32)
        count = C.c_size_t(99)
        st = L.gf_file_interp_tiles(f._h, _ptr(spec), drows.size, _ptr(drows), _ptr(dcols), _ptr(tiles) if cap else None, cap, C.byref(count))
        assert st == OK and count.value == wantw.size
        assert tiles[:min(cap, wantw.size)].tolist() == wantw[:min(cap, wantw.size)].tolist() and (tiles[min(cap, wantw.size):] == -7).all()


def test_tiles_argument_errors(opened):
    L = _lib.lib()
    f = opened[15]
    rows, cols = np.zeros(2, np.int32), np.zeros(2, np.int32)
    drows, dcols = np.zeros(2), np.zeros(2)
    tiles, n = np.zeros(4, np.int32), C.c_size_t()
    spec = f.points_spec(0)
    assert L.gf_file_cells_tiles(None, 2, _ptr(rows), _ptr(cols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_cells_tiles(f._h, 2, None, _ptr(cols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_cells_tiles(f._h, 2, _ptr(rows), None, _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_cells_tiles(f._h, 2, _ptr(rows), _ptr(cols), None, 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_cells_tiles(f._h, 2, _ptr(rows), _ptr(cols), _ptr(tiles), 4, None) == ERR_ARG
    assert L.gf_file_cells_tiles(f._h, 0, None, None, None, 0, C.byref(n)) == OK and n.value == 0
    assert L.gf_file_interp_tiles(None, _ptr(spec), 2, _ptr(drows), _ptr(dcols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_tiles(f._h, None, 2, _ptr(drows), _ptr(dcols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_tiles(f._h, _ptr(spec), 2, None, _ptr(dcols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert L.gf_file_interp_tiles(f._h, _ptr(spec), 2, _ptr(drows), _ptr(dcols), _ptr(tiles), 4, None) == ERR_ARG
    for field, value in (("wrap", 3), ("wrap", -1), ("target", 3), ("target", -1)):
        bad = f.points_spec(0)
        bad[field] = value
        assert L.gf_file_interp_tiles(f._h, _ptr(bad), 2, _ptr(drows), _ptr(dcols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    small = gridfour_amd.GvrsFileHip(K.image_of((3, 9, 3, 3)))                    # a grid under 4 x 4: the reference's constructor throws
    assert L.gf_file_interp_tiles(small._h, _ptr(small.points_spec(0)), 2, _ptr(drows), _ptr(dcols), _ptr(tiles), 4, C.byref(n)) == ERR_ARG
    assert small.cells_tiles([2], [8]).tolist() == [2]


def test_reads_refuse_their_arguments_without_a_context(opened):
    """every GF_ERR_ARG case is answered before the context or a device is looked at: with a NULL context the answer is GF_ERR_ARG"""
    L = _lib.lib()
    f = opened[15]
    image = f.image
    rows, cols, drows, dcols = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2), np.zeros(2)
    value, status, z, n = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2), C.c_size_t()
    values = (C.c_void_p * 1)(value.ctypes.data)
    spec = f.points_spec(0)
    out = np.zeros(1, gridfour_amd.codec._INTERP_OUT)
    out["z"] = z.ctypes.data
    for name in ("gf_file_read_points_elems_dev", "gf_file_read_points_elems"):
        fn = getattr(L, name)
        assert fn(None, f._h, _ptr(image), image.size, 2, _ptr(rows), _ptr(cols), 1, 4, values, _ptr(status), C.byref(n)) == ERR_ARG
        assert fn(None, f._h, _ptr(image), image.size, 0, None, None, 1, 0, values, _ptr(status), C.byref(n)) == ERR_ARG
        assert fn(None, None, None, 0, 2, None, None, 1, 4, None, None, None) == ERR_ARG
    for name in ("gf_file_interp_points_dev", "gf_file_interp_points"):
        fn = getattr(L, name)
        assert fn(None, f._h, _ptr(image), image.size, 0, _ptr(spec), 2, _ptr(drows), _ptr(dcols), None, 1, 4, _ptr(out), C.byref(n)) == ERR_ARG
        assert fn(None, f._h, _ptr(image), image.size, 1, _ptr(spec), 2, _ptr(drows), _ptr(dcols), None, 1, 4, _ptr(out), C.byref(n)) == ERR_ARG
        assert fn(None, f._h, _ptr(image), image.size, -1, _ptr(spec), 2, _ptr(drows), _ptr(dcols), None, 1, 4, _ptr(out), C.byref(n)) == ERR_ARG
        assert fn(None, None, None, 0, 0, None, 2, None, None, None, 1, 4, None, None) == ERR_ARG
