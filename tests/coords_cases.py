"""The cases the tests of the queries at coordinates share (test_coords_ref.py, test_coords_program.py, test_file_coords_host.py,
test_gpu_file_coords.py): four small grids with tiles of 5 x 5 -- three geographic (the longitudes wrap, bracket, cover a limited
range) and one Cartesian whose m2r has a negative row scale and offsets, or is a rotation -- their file images with one tile
absent and one record damaged, and the query points: every cell edge with its neighbouring doubles, the longitudes that take each
retry of mapGeographicToGridPoint, the neighbours of both fringes, the latitude check's edges, NaN and infinities, and sixteen
latitudes on which fdlibm's cosine and the host libm's differ."""
import math

import numpy as np

import coords_ref as CR
import gvrs_file_build as B

FILL = -9999
LATS = (-82.5, 15.0, 12)                                     # y0, cell height, rows: -82.5 ... 82.5

# latitudes on which coords_ref.strict_cos(to_radians(lat)) != math.cos(to_radians(lat)), by exactly 1 ulp: found once among
# random.seed(20261021) uniform(-90, 90) draws, two of each sign from each of |lat| in [0, 17), [17, 45), [45, 70), [70, 90)
COS_TELLING = [13.617882402587952, 14.588479208550751, -5.272109680632198, -12.969118259873, 27.28211365839924, 28.98178961399634,
               -43.52963270236965, -31.553442363866715, 62.42148220459907, 63.75707098794044, -58.92644285507076, -46.38149126217299,
               73.24417050692793, 72.1653266357815, -84.83833971136407, -79.24461478307067]


def geo_facts(x0, cell_x, n_cols):
    y0, cell_y, n_rows = LATS
    x1, y1 = x0 + (n_cols - 1) * cell_x, y0 + (n_rows - 1) * cell_y
    m00, m11 = 1 / cell_x, 1 / cell_y
    return dict(coordinate_system=2, domain=(x0, y0, x1, y1), cell_size=(cell_x, cell_y), m2r=(m00, 0.0, -x0 * m00, 0.0, m11, -y0 * m11),
                r2m=(cell_x, 0.0, x0, 0.0, cell_y, y0))


def cart_facts(rotation=False):
    """rows run against y (a negative row scale) from offsets that are no multiples of the cell; or m2r is a rotation by 30 degrees"""
    if rotation:
        c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
        return dict(coordinate_system=1, domain=(0.0, 0.0, 10.0, 8.0), cell_size=(1.0, 1.0), m2r=(c, -s, 1.25, s, c, -0.5),
                    r2m=(c, s, -1.25 * c + 0.5 * s, -s, c, 1.25 * s + 0.5 * c))
    return dict(coordinate_system=1, domain=(100.3, 56.1, 120.3, 60.1), cell_size=(2.0, 0.5), m2r=(0.5, 0.0, -50.15, 0.0, -2.0, 120.2),
                r2m=(2.0, 0.0, 100.3, 0.0, -0.5, 60.1))


GRIDS = {                                                    # name: (grid, element kinds, header facts, absent tile, damaged tile)
    "wraps": ((12, 12, 5, 5), ("int",), geo_facts(-180.0, 30.0, 12), 4, 2),
    "brackets": ((12, 13, 5, 5), ("int",), geo_facts(-180.0, 30.0, 13), 4, 6),
    "limited": ((12, 10, 5, 5), ("int", "float"), geo_facts(10.0, 3.0, 10), 3, 0),
    "cart": ((9, 11, 5, 5), ("short",), cart_facts(), 1, 5),
    "rotated": ((9, 11, 5, 5), ("short",), cart_facts(True), 1, 5),
}
GEO = ("wraps", "brackets", "limited")
WRAP = {"wraps": 1, "brackets": 2, "limited": 0, "cart": 0, "rotated": 0}


def info_of(name):
    """the coordinate facts as GvrsFileHip.info holds them (what coords_ref.Coords reads)"""
    grid, _, facts, _, _ = GRIDS[name]
    x0, y0, x1, y1 = facts["domain"]
    return dict(grid=grid, coordinate_system=facts["coordinate_system"], x0=x0, y0=y0, x1=x1, y1=y1, cell_size_x=facts["cell_size"][0],
                cell_size_y=facts["cell_size"][1], m2r=facts["m2r"], r2m=facts["r2m"])


def coords_of(name):
    return CR.Coords(info_of(name))


def image_of(name):
    """(the file image, the same with a body byte of the damaged tile's record changed, {tile: position}, the planes per element)"""
    grid, kinds, facts, absent, damaged = GRIDS[name]
    n_tile_rows, n_tile_cols = -(-grid[0] // 5), -(-grid[1] // 5)
    rng = np.random.default_rng(len(name))
    shape = (n_tile_rows * 5, n_tile_cols * 5)
    planes, elements = [], []
    for k, kind in enumerate(kinds):
        if kind == "float":
            p = rng.normal(0.0, 300.0, shape).astype(np.float32)
            elements.append(B.element("f%d" % k, "float"))
        else:
            p = rng.integers(-3000, 3000, shape).astype(np.int16 if kind == "short" else np.int32)
            p[rng.integers(0, 40, shape) == 0] = FILL
            elements.append(B.element("e%d" % k, kind, fill=FILL))
        planes.append(p)
    records = {}
    for t in range(n_tile_rows * n_tile_cols):
        if t != absent:
            r, c = divmod(t, n_tile_cols)
            records[t] = B.standard_record(t, [p[r * 5:r * 5 + 5, c * 5:c * 5 + 5] for p in planes])
    image, named = B.build_image(grid, elements, records, **facts)
    at = named[damaged] + 9
    bad = image[:at] + bytes([image[at] ^ 0x40]) + image[at + 1:]
    return image, bad, named, planes


def around(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def file_points(name):
    """(x, y) as z() reads them, a few hundred; the first 65 hold the edges of the rules"""
    grid, _, facts, _, _ = GRIDS[name]
    co = coords_of(name)
    n_rows, n_cols = grid[0], grid[1]
    rng = np.random.default_rng(7 + len(name))
    pts = []
    if name in GEO:
        x0, y0 = co.x0, co.y0
        mid_lat, mid_lon = y0 + 4.3 * co.csy, x0 + 3.7 * co.csx
        # the latitude check's edges, NaN and infinities, the longitudes of the issue's list
        for lat in (90.0, -90.0, 90.0001, -90.0001, np.nextafter(90.0001, np.inf), np.nextafter(-90.0001, -np.inf), 91.0, -1e300):
            pts.append((mid_lon, lat))
        for x, y in ((np.nan, mid_lat), (mid_lon, np.nan), (np.inf, mid_lat), (-np.inf, mid_lat), (mid_lon, np.inf), (mid_lon, -np.inf), (np.nan, np.nan)):
            pts.append((x, y))
        for lon in (x0, x0 + 360, x0 - 360, x0 + 540, x0 - 540, 179.999999, 180.0, -180.0, -0.0, 0.0, x0 - 20.0, x0 + 200.0, 1e300):
            pts.append((lon, mid_lat))
        # the neighbours of both fringes on both axes, also a turn away
        for f in co.col_fringe:
            for v in around(f):
                for turn in (0.0, 360.0, -360.0):
                    pts.append((x0 + v * co.csx + turn, mid_lat))
        for f in co.row_fringe:
            for v in around(f):
                pts.append((mid_lon, y0 + v * co.csy))
        for lat in COS_TELLING:
            pts.append((x0 + rng.uniform(0, n_cols - 1) * co.csx, lat))
        # every column and row edge with its neighbours
        for k in range(n_cols + 1):
            for v in around(x0 + (k - 0.5) * co.csx):
                pts.append((v, mid_lat))
        for k in range(n_rows + 1):
            for v in around(y0 + (k - 0.5) * co.csy):
                pts.append((mid_lon, v))
        while len(pts) < 300:
            pts.append((rng.uniform(-400.0, 400.0), rng.uniform(-90.0, 90.0)))
    else:
        def model(row, col):
            return co.grid_to_model(row, col)
        for x, y in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (1e300, 1.0), (1.0, -1e300)):
            pts.append((x, y))
        for f in co.row_fringe:
            for v in around(f):
                pts.append(model(v, 3.3))
        for f in co.col_fringe:
            for v in around(f):
                pts.append(model(2.2, v))
        for k in range(n_cols + 1):
            x, y = model(4.4, k - 0.5)
            for v in around(x):
                pts.append((v, y))
        for k in range(n_rows + 1):
            x, y = model(k - 0.5, 5.5)
            for v in around(y):
                pts.append((x, v))
        pts.append((1000.0, 95.0))                               # |y| > 90.0001 is no latitude here: never refused
        while len(pts) < 300:
            pts.append(model(rng.uniform(-1.0, n_rows), rng.uniform(-1.0, n_cols)))
    x, y = np.array([p[0] for p in pts], np.float64), np.array([p[1] for p in pts], np.float64)
    return x, y


def grid_points(name):
    """(row, col) for the queries in grid coordinates: a lattice at half-cell offsets over the grid and its fringe, the fringes'
    neighbours, NaN and infinities, rows whose latitude the check refuses (geographic grids)"""
    grid = GRIDS[name][0]
    co = coords_of(name)
    r, c = np.meshgrid(np.arange(-1.0, grid[0] + 0.5, 0.75), np.arange(-1.0, grid[1] + 0.5, 0.5), indexing="ij")
    rows, cols = r.ravel().tolist(), c.ravel().tolist()
    for f in co.row_fringe:
        for v in around(f):
            rows.append(v), cols.append(2.5)
    for f in co.col_fringe:
        for v in around(f):
            rows.append(3.5), cols.append(v)
    for row, col in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (1e300, 2.0), (-40.0, 2.0), (11.6, 2.0)):
        rows.append(row), cols.append(col)
    return np.array(rows, np.float64), np.array(cols, np.float64)


COUNTS = (1, 63, 64, 65, 257)                                # a lone lane, the wave seam, the grid-stride seam of the mark kernel
