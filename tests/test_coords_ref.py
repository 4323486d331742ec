"""The restatement coords_ref.py held to what can be known without the C++: the cosine's known values and the 1-ulp condition
Java gives Math.cos, the case set's power to tell fdlibm's cosine from a libm's, Angle.to180 / to360 at every branch, the wrap and
bracket decision, the retries of mapGeographicToGridPoint -- and gf_file_interp_spec against the restatement's derivation on the
reference's fifteen sample files."""
import math

import numpy as np
import pytest

import gridfour_amd

import coords_cases as K
import coords_ref as R
from test_file_open import sample_path


def ulps_apart(a, b):
    """the distance of two doubles of one sign in units of the last place of the larger magnitude"""
    assert (a >= 0) == (b >= 0)
    return abs(R.bits(abs(a)) - R.bits(abs(b)))


def test_cosine_known_values():
    assert R.strict_cos(0.0) == 1.0 and R.strict_cos(-0.0) == 1.0
    for x in (1e-9, 0.1, 0.29, 0.31, 0.5, 0.78, 0.79, 1.0, 1.5, 1.5707963, 1.6, 2.3):
        assert R.strict_cos(x) == R.strict_cos(-x)                       # even, through every branch
    a, b = R.strict_cos(R.to_radians(90.0)), R.strict_cos(R.to_radians(-90.0))
    assert a == b and a > 0
    assert R.hi(R.to_radians(90.0)) == 0x3ff921fb                         # ... by the second-term retry of the reduction
    assert R.strict_cos(R.to_radians(90.0001)) < 0
    co = K.coords_of("wraps")
    assert co.col_spacing(co.du, 90.0001) == 1.0 and co.col_spacing(co.du, 90.0) == 1.0   # dx < 1 -> 1
    assert co.col_spacing(co.du, 0.0) == co.du
    assert math.isnan(R.strict_cos(float("nan"))) and math.isnan(R.strict_cos(float("inf"))) and math.isnan(R.strict_cos(2.4))


def case_latitudes():
    lats = []
    for name in K.GEO:
        _, y = K.file_points(name)
        lats += [v for v in y.tolist() if abs(v) <= 90.0001]
    return lats


def test_cosine_within_one_ulp_of_libm_on_every_case_latitude():
    """the contract Java gives Math.cos, as a condition: two functions each under 1 ulp from the true value are not 2 apart"""
    lats = case_latitudes()
    assert len(lats) > 600
    for lat in lats:
        x = R.to_radians(lat)
        assert ulps_apart(R.strict_cos(x), math.cos(x)) <= 1, lat


def test_the_cases_tell_the_two_cosines_apart():
    assert len(K.COS_TELLING) == len(set(K.COS_TELLING)) == 16
    for lat in K.COS_TELLING:
        x = R.to_radians(lat)
        assert R.strict_cos(x) != math.cos(x), lat
    for name in K.GEO:                                                   # ... and every geographic grid's points hold them
        _, y = K.file_points(name)
        assert set(K.COS_TELLING) <= set(y.tolist())
        co = K.coords_of(name)
        # (the product with du rounds once more and can absorb the ulp: one latitude whose SPACING differs is what parity needs)
        assert sum(co.col_spacing(co.du, lat) != max(1.0, math.cos(R.to_radians(lat)) * co.du) for lat in K.COS_TELLING) >= 1


def same(a, b):
    return R.bits(a) == R.bits(b)


def test_to180_to360():
    nz = -0.0
    for a, w180, w360 in ((0.0, 0.0, 0.0), (nz, 0.0, 0.0), (180.0, -180.0, 180.0), (-180.0, -180.0, 180.0), (360.0, 0.0, 0.0), (-360.0, 0.0, 0.0),
                          (540.0, -180.0, 180.0), (-540.0, -180.0, 180.0), (190.0, -170.0, 190.0), (-190.0, 170.0, 170.0), (10.0, 10.0, 10.0),
                          (-10.0, -10.0, 350.0), (179.0, 179.0, 179.0), (-181.0, 179.0, 179.0), (725.0, 5.0, 5.0)):
        assert same(R.to180(a), w180), a
        assert same(R.to360(a), w360), a
    for a in (float("inf"), float("-inf"), float("nan")):
        assert math.isnan(R.to180(a)) and math.isnan(R.to360(a))
    assert same(R.to180(np.nextafter(180.0, 0.0)), np.nextafter(180.0, 0.0)) and same(R.to180(np.nextafter(-180.0, -np.inf)), 360 + np.nextafter(-180.0, -np.inf))


def wrap_of(x0, x1, cell):
    info = K.info_of("wraps")
    info.update(x0=x0, x1=x1, cell_size_x=cell)
    return R.Coords(info).wrap


def test_wrap_and_bracket_decision():
    assert wrap_of(-180.0, 180.0, 30.0) == 2                              # 360 wide: brackets
    assert wrap_of(-180.0, 150.0, 30.0) == 1                              # one cell short of 360: wraps
    assert wrap_of(-180.0, 150.0 + 1e-7, 30.0) == 1                       # ... within 1e-6
    assert wrap_of(-180.0, 150.0 + 1e-5, 30.0) == 0                       # ... not within
    assert wrap_of(10.0, 37.0, 3.0) == 0                                  # limited coverage
    assert [K.coords_of(n).wrap for n in ("wraps", "brackets", "limited", "cart", "rotated")] == [1, 2, 0, 0, 0]
    info = K.info_of("brackets")
    info["coordinate_system"] = 1                                        # the decision is taken for a geographic file only
    assert R.Coords(info).wrap == 0


def test_every_retry_of_the_longitude_is_taken():
    for name in K.GEO:
        co = K.coords_of(name)
        x, y = K.file_points(name)
        took = []
        for lon, lat in zip(x.tolist(), y.tolist()):
            co.geo_to_grid(lat, lon, took)
        assert set(took) == {0, 1, 2}, name
        # both sides of both column fringes, directly and through each retry
        cols = np.array([co.geo_to_grid(lat, lon)[1] for lon, lat in zip(x.tolist(), y.tolist())])
        f0, f1 = co.col_fringe
        took = np.array(took)
        for b in (0, 1, 2):
            if (name, b) == ("limited", 2):                              # (columns under 180 degrees from x0: where to360 lands
                continue                                                 # inside, to180 has landed there before it)
            inside = (cols >= f0) & (cols <= f1) & (took == b)
            assert inside.any(), (name, b)
        if name == "limited":                                            # (a grid around the globe has a column for every longitude)
            assert ((cols < f0) | (cols > f1)).any()                    # ... and outside after all three


def test_grid_point_fringe_and_saturation():
    co = K.coords_of("wraps")
    f0, f1 = co.row_fringe
    assert co.grid_point(f0, f1)[0] == 0 and co.grid_point(np.nextafter(f0, -np.inf), 0.0)[0] == -1
    assert co.grid_point(f1, 0.0)[0] == 11 and co.grid_point(np.nextafter(f1, np.inf), 0.0)[0] == 12
    assert co.grid_point(float("nan"), float("inf")) == (0, 2147483647) and co.grid_point(-1e300, 3.4999)[0] == -2147483648
    assert co.grid_point(2.5, 3.4999) == (3, 3)


@pytest.mark.parametrize("k", range(15))
def test_sample_files_interp_spec(golden_dir, k):
    """the samples are Cartesian or unset: they pin the fringes and du / dv = the cell sizes"""
    f = gridfour_amd.GvrsFileHip(sample_path(golden_dir, k))
    co = R.Coords(f.info)
    assert f.info["coordinate_system"] in (0, 1) and co.wrap == 0
    for e in range(f.n_elems):
        for target in (0, 1, 2):
            s = f.coords_spec(e, target)
            el = f.info["elems"][e]
            assert (int(s["n_rows_grid"][0]), int(s["n_cols_grid"][0])) == f.grid[:2] and s["block"][0].tolist() == [0, 0, f.grid[0], f.grid[1]]
            assert (int(s["elem_type"][0]), int(s["fill_i"][0]), int(s["wrap"][0]), int(s["target"][0])) == (el["type"], el["fill_i"], 0, target)
            got = [float(s[n][0]) for n in ("row_spacing", "col_spacing", "row_fringe0", "row_fringe1", "col_fringe0", "col_fringe1")]
            want = [co.dv, co.du, co.row_fringe[0], co.row_fringe[1], co.col_fringe[0], co.col_fringe[1]]
            assert [R.bits(v) for v in got] == [R.bits(v) for v in want]
            assert got[0] == f.info["cell_size_y"] and got[1] == f.info["cell_size_x"]
            assert got[2] < -0.5 and got[3] > f.grid[0] - 0.5
