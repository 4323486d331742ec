"""The cases the CPU tests of the reads at points share (test_file_points_host.py through the library, test_file_points_program.py
through the stand-alone program): grids, cells and query points chosen for the edges of the arithmetic -- every grid edge and one
cell outside it, windows that take columns from both ends of the grid under wrap 1 and 2, NaN coordinates, points outside the
fringe, tiles narrower and shorter than a window."""
import numpy as np

import gvrs_file_build as B

RANK_CHUNK_WORDS = 1024                                       # GF_POINTS_RANK_CHUNK of gvrs_kernels.h: the bitmap words a turn of k_points_rank takes
GRID299 = (45, 37, 2, 3)                                     # 23 x 13 tiles of 2 x 3 cells: a window spans up to 3 x 2 of them
SAMPLE_GRIDS = [(10, 10, 5, 5), (100, 100, 50, 50), (10, 10, 6, 6), (11, 11, 11, 11), (101, 101, 101, 101)]
EXTRA_GRIDS = [GRID299, (5, 4, 1, 1), (9, 6, 4, 2), (7, 260, 3, 1)]   # ... 1 x 1 tiles (16 tiles a window), a 4-column grid's relatives, > 8 words


def image_of(grid, held=None, seed=5):
    """a small file image over grid with one int element; held: the tiles that have a record (default: two in three)"""
    n_tile_rows, n_tile_cols = -(-grid[0] // grid[2]), -(-grid[1] // grid[3])
    rng = np.random.default_rng(seed)
    held = [t for t in range(n_tile_rows * n_tile_cols) if rng.integers(0, 3) != 0] if held is None else held
    records = {t: B.standard_record(t, [np.full((grid[2], grid[3]), t, np.int32)]) for t in held}
    image, _ = B.build_image(grid, [B.element("z", "int")], records)
    return image


def cell_points(grid, seed=1):
    """every grid corner and edge midpoint, one cell outside each edge, far outside, and scattered cells with duplicates"""
    nr, nc = grid[0], grid[1]
    rng = np.random.default_rng(seed)
    rows = [0, 0, nr - 1, nr - 1, nr // 2, nr // 2, 0, nr - 1, -1, nr, 0, 0, -1, nr, 2 ** 31 - 1, -2 ** 31, 0]
    cols = [0, nc - 1, 0, nc - 1, 0, nc - 1, nc // 2, nc // 2, 0, 0, -1, nc, -1, nc, 0, 0, 2 ** 31 - 1]
    r, c = rng.integers(0, nr, 40), rng.integers(0, nc, 40)
    rows, cols = rows + r.tolist() + r[:7].tolist(), cols + c.tolist() + c[:7].tolist()
    return np.array(rows, np.int32), np.array(cols, np.int32)


def window_points(grid, seed=2):
    """a lattice at half-cell offsets over the grid and its fringe (thinned for the large grids), the columns that wrap takes from
    both ends, points on and just outside the fringe, NaN coordinates, far away points"""
    nr, nc = grid[0], grid[1]
    step_r, step_c = max(1, nr // 12), max(1, nc // 12)
    r, c = np.meshgrid(np.arange(-1.0, nr + 0.5, 0.5 * step_r), np.arange(-1.0, nc + 0.5, 0.5 * step_c), indexing="ij")
    rows, cols = r.ravel().tolist(), c.ravel().tolist()
    for col in (-0.5, 0.25, nc - 0.75, -1.0, -2.5, -3.0, nc - 1.0, nc - 0.5, nc + 0.0, nc + 0.5, 1.0, nc - 3.0, nc - 2.0):
        for row in (0.0, 1.5, nr - 1.0, nr - 2.5):
            rows.append(row)
            cols.append(col)
    for row, col in ((-0.5, 2.0), (-0.5000001, 2.0), (nr - 0.5, 2.0), (nr - 0.4999, 2.0), (2.0, -0.5), (2.0, -0.5000001), (2.0, nc - 0.5),
                     (2.0, nc - 0.4999), (float("nan"), 1.0), (1.0, float("nan")), (1e300, 1.0), (1.0, -1e300), (float("inf"), 1.0),
                     (1.0, float("-inf")), (3e9, 3e9)):
        rows.append(row)
        cols.append(col)
    return np.array(rows, np.float64), np.array(cols, np.float64)


FRINGES = [None, ((-0.75, 0.25), (-1.5, 0.75))]               # the default, and one widened below and above: (row, col) offsets


def fringe_of(grid, k):
    if FRINGES[k] is None:
        return None, None
    (r0, r1), (c0, c1) = FRINGES[k]
    return (-0.5 + r0, grid[0] - 0.5 + r1), (-0.5 + c0, grid[1] - 0.5 + c1)
