"""GVRS files queried at coordinates on the GPU (gf_file_map_points_dev: k_coords_map; gf_file_interp_coords[_dev]: the coordinate
instantiations of k_points_mark and k_points_interp), on the four small grids of coords_cases.py -- longitudes that wrap, bracket
and cover a limited range, and a Cartesian grid with a negative row scale or a rotation -- each with one tile absent and one
record damaged.  The mapping kernel is held to the host form bit for bit; the fused interpolation is held, bit for bit and NaN
payloads included, to the route it fuses: gf_file_interp_points_dev fed the rows, columns and spacings of the Python restatement
coords_ref.py (whose cosine is fdlibm's: a libm cosine in the kernel would differ on the sixteen telling latitudes)."""
import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import _lib, GvrsFileHip

import coords_cases as K
import coords_ref as CR

pytestmark = pytest.mark.gpu
OK, DECLINED, ERR_FORMAT, ERR_ARG, ERR_CAPACITY = _lib.OK, _lib.DECLINED, _lib.ERR_FORMAT, _lib.ERR_ARG, _lib.ERR_CAPACITY


@pytest.fixture(scope="module")
def ctx():
    return gridfour_amd.GvrsHipContext()


@pytest.fixture(scope="module")
def files():
    """name: (the file, the image with the damaged record, the restatement's rules)"""
    out = {}
    for name in K.GRIDS:
        image, bad, _, _ = K.image_of(name)
        f = GvrsFileHip(image)
        out[name] = (f, bad, CR.Coords(f.info))
    return out


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_or_nan(a, want):
    a, want = np.asarray(a, np.float64), np.asarray(want, np.float64)
    return bool(((u64(a) == u64(want)) | (np.isnan(a) & np.isnan(want))).all())


def points_of(name, kind):
    return K.file_points(name) if kind == CR.COORDS_FILE else K.grid_points(name)


_restated = {}


def restated(name, kind, co):
    """the restatement's (status, rows, cols, spacings) of a grid's points, computed once and shared"""
    if (name, kind) not in _restated:
        a, b = points_of(name, kind)
        q = [co.query(kind, p, r) for p, r in zip(a.tolist(), b.tolist())]
        _restated[name, kind] = tuple(np.array([v[k] for v in q], np.int32 if k == 0 else np.float64) for k in range(4))
    return _restated[name, kind]


# ---- 1. the mapping kernel against the host form ----
@pytest.mark.parametrize("name", list(K.GRIDS))
def test_map_points_dev_is_the_host_form(ctx, files, name):
    f, _, co = files[name]
    x, y = K.file_points(name)
    rows, cols = K.grid_points(name)
    for kind, (a, b) in ((CR.GEO_TO_GRID, (x, y)), (CR.MODEL_TO_GRID, (x, y)), (CR.GRID_TO_GEO, (rows, cols)), (CR.GRID_TO_MODEL, (rows, cols))):
        want, got = f.map_points(kind, a, b), f.map_points_dev(ctx, kind, a, b)
        assert sorted(got) == sorted(want)
        for k in want:
            if want[k].dtype == np.float64:
                assert np.array_equal(u64(got[k]), u64(want[k])), (kind, k)
            else:
                assert np.array_equal(got[k], want[k]), (kind, k)
    took = []
    if name in K.GEO:
        for lon, lat in zip(x.tolist(), y.tolist()):
            co.geo_to_grid(lat, lon, took)
        assert set(took) == {0, 1, 2}                                     # every retry of the longitude ran on the device
        assert (f.map_points_dev(ctx, CR.GEO_TO_GRID, x, y)["status"] == ERR_ARG).any()


@pytest.mark.parametrize("n", K.COUNTS)
def test_map_points_dev_counts(ctx, files, n):
    f, _, _ = files["brackets"]
    x, y = K.file_points("brackets")
    want, got = f.map_points(CR.GEO_TO_GRID, x[:n], y[:n]), f.map_points_dev(ctx, CR.GEO_TO_GRID, x[:n], y[:n])
    for k in want:
        assert got[k].size == n and got[k].tobytes() == want[k].tobytes(), k


# ---- 2., 3. the fused interpolation against the two calls it replaces ----
def check_fused(ctx, f, image, co, name, kind, e, target, n=None, caller_spacing=False, forms=("dev",)):
    a, b = points_of(name, kind)
    st, rows, cols, spacing = restated(name, kind, co)
    n = a.size if n is None else n
    a, b, st, rows, cols, spacing = a[:n], b[:n], st[:n], rows[:n], cols[:n], spacing[:n]
    spec = f.coords_spec(e, target)
    cs = None
    if caller_spacing:
        cs = np.random.default_rng(n).uniform(0.5, 900.0, n)
        cs[::11] = 0.0                                                   # a zero spacing: GF_ERR_ARG for the point with target >= FIRST
        spacing = np.where(st == CR.OK, cs, np.nan)
    # the unfused route: the parent's entry point on rows, columns and spacings mapped beforehand (a refused point: NaN coordinates,
    # which that entry point answers with GF_ERR_ARG and NaN outputs)
    want, _ = f.interp_points_dev(ctx, e, spec, rows, cols, spacing, True, image=image)
    touched = f.interp_coords_tiles(kind, spec, a, b).size
    got = None
    for form in forms:
        read = f.interp_coords_dev if form == "dev" else f.interp_coords
        res, n_touched = read(ctx, e, kind, spec, a, b, cs, True, image=image)
        assert n_touched == touched, form
        assert sorted(res) == sorted(list(want) + ["col_spacing_used"])
        assert np.array_equal(res["status"], want["status"]), form
        for k in want:
            if k != "status":
                assert np.array_equal(u64(res[k]), u64(want[k])), (form, k)
        assert same_or_nan(res["col_spacing_used"], spacing), form
        refused = st != CR.OK
        assert (res["status"][refused] == ERR_ARG).all() and np.isnan(res["z"][refused]).all() and np.isnan(res["col_spacing_used"][refused]).all()
        got = got or res
    return got, st


CASES = [(name, kind, e) for name in K.GRIDS for kind in (CR.COORDS_FILE, CR.COORDS_GRID) for e in range(len(K.GRIDS[name][1]))]


@pytest.mark.parametrize("name,kind,e", CASES)
def test_interp_coords_dev_is_map_then_interp(ctx, files, name, kind, e):
    f, bad, co = files[name]
    for target in (0, 1, 2):
        res, st = check_fused(ctx, f, bad, co, name, kind, e, target)
        s = res["status"]
        assert (s == OK).any() and (s == DECLINED).any() and (s == ERR_ARG).any()
        assert (s == ERR_FORMAT).any()                                   # windows over the damaged record: the failed-tile path
        assert (st != CR.OK).any() == (name in K.GEO)                    # the latitude check refuses on geographic files only
        ok = s == OK
        assert np.isnan(res["z"][ok]).any() and (~np.isnan(res["z"][ok])).any()   # fill cells and the absent tile read as NaN
        if target >= 1 and name in K.GEO and kind == CR.COORDS_FILE:
            used = res["col_spacing_used"]
            assert (used[~np.isnan(used)] >= 1.0).all() and (used == 1.0).any() and (used > 1000.0).any()   # the clamp, and real spacings


@pytest.mark.parametrize("name,kind,e", CASES)
def test_interp_coords_dev_with_the_callers_spacings(ctx, files, name, kind, e):
    f, bad, co = files[name]
    for target in (1, 2):
        res, _ = check_fused(ctx, f, bad, co, name, kind, e, target, caller_spacing=True)
        assert (res["status"] == OK).any()


@pytest.mark.parametrize("n", K.COUNTS)
def test_interp_coords_counts(ctx, files, n):
    f, bad, co = files["wraps"]
    check_fused(ctx, f, bad, co, "wraps", CR.COORDS_FILE, 0, 1, n=n)
    f, bad, co = files["rotated"]
    check_fused(ctx, f, bad, co, "rotated", CR.COORDS_FILE, 0, 2, n=n)


# ---- 4. capacity ----
def test_capacity(ctx, files):
    f, bad, co = files["limited"]
    x, y = K.file_points("limited")
    spec = f.coords_spec(1, 1)
    n = f.interp_coords_tiles(CR.COORDS_FILE, spec, x, y).size
    assert n > 1
    for read in (f.interp_coords_dev, f.interp_coords):
        res, touched = read(ctx, 1, CR.COORDS_FILE, spec, x, y, max_tiles=n)
        assert touched == n and (res["status"] == OK).any()
        res, touched, code = read(ctx, 1, CR.COORDS_FILE, spec, x, y, max_tiles=n - 1, return_code=True)
        assert code == ERR_CAPACITY and touched == n
        assert all((v.view(np.uint8) == 0x7f).all() for v in res.values())               # every output byte as pre-set
        with pytest.raises(gridfour_amd.GvrsHipError) as err:
            read(ctx, 1, CR.COORDS_FILE, spec, x, y, max_tiles=n - 1)
        assert err.value.status == ERR_CAPACITY
    # points that touch nothing -- refused, NaN, outside the fringe -- need no room
    res, touched = f.interp_coords_dev(ctx, 0, CR.COORDS_FILE, spec, [20.0, np.nan, 100.0], [95.0, 0.0, 0.0], max_tiles=0)
    assert touched == 0 and res["status"].tolist() == [ERR_ARG, ERR_ARG, DECLINED] and np.isnan(res["z"]).all()
    assert np.isnan(res["col_spacing_used"][0]) and not np.isnan(res["col_spacing_used"][2])
    res, touched = f.interp_coords_dev(ctx, 0, CR.COORDS_FILE, spec, [], [])
    assert touched == 0 and res["z"].size == 0 and res["col_spacing_used"].size == 0


# ---- 5. the host form ----
@pytest.mark.parametrize("name", list(K.GRIDS))
def test_the_host_form_is_the_device_form(ctx, files, name):
    f, bad, co = files[name]
    check_fused(ctx, f, bad, co, name, CR.COORDS_FILE, 0, 2, forms=("dev", "host"))
    check_fused(ctx, f, bad, co, name, CR.COORDS_GRID, 0, 1, caller_spacing=True, forms=("dev", "host"))


# ---- 6. cells at coordinates ----
@pytest.mark.parametrize("name", list(K.GRIDS))
def test_read_coords_is_the_block_at_the_grid_point(ctx, files, name):
    f, bad, co = files[name]
    blocks, status, _ = f.read_block_dev(ctx, (0, 0, f.grid[0], f.grid[1]), True, image=bad)
    x, y = K.file_points(name)
    values, st, mapped = f.read_coords(ctx, x, y, image=bad)
    kind = CR.GEO_TO_GRID if name in K.GEO else CR.MODEL_TO_GRID
    want = [co.map_point(kind, p, q) for p, q in zip(x.tolist(), y.tolist())]
    assert mapped.tolist() == [m[5] for m in want]
    irow, icol = np.array([m[2] for m in want]), np.array([m[3] for m in want])
    inside = (mapped == OK) & (irow >= 0) & (irow < f.grid[0]) & (icol >= 0) & (icol < f.grid[1])
    assert inside.any() and (~inside).any()
    across = -(-f.grid[1] // 5)
    for e in range(f.n_elems):
        assert (st[e][~inside] == ERR_ARG).all()                          # a GridPoint outside the grid, or a refused point
        tile = (irow[inside] // 5) * across + icol[inside] // 5
        assert np.array_equal(st[e][inside], status[e][tile])
        assert values[e][inside].tobytes() == blocks[e][irow[inside], icol[inside]].tobytes()
        assert (st[e][inside] == ERR_FORMAT).any() and (st[e][inside] == OK).any()
