"""CPU-only: the numpy model of the reference's B-spline interpolator (tests/interp_ref.py) pinned by answers that can be checked
by hand with the reference's operation order (interpolation/InterpolatorBSpline.java:192-378, gvrs/GvrsInterpolatorBSpline.java:
374-484), by its window rules at every edge, and by the surface and tolerances of the reference's own InterpolationBSplineTest."""
import numpy as np

import interp_ref as R

RAMP = (4.0 * np.arange(4)[:, None] + np.arange(4)[None, :]).astype(np.float32)          # z = 4 * row + col on a 4 x 4 grid


def _one(spec, block, row, col, cs=None):
    out = R.interp(spec, block, [row], [col], None if cs is None else [cs])
    return {k: (v[0] if k != "normal" else v[0]) for k, v in out.items()}


def test_hand_checked_values_on_the_ramp():
    spec = R.Spec(4, 4)
    assert _one(spec, RAMP, 1.0, 1.0)["z"] == 5.0
    assert _one(spec, RAMP, 1.25, 1.5)["z"] == 6.5
    # the corner: both outer-band adjustments of interpolate, u = -1 and v = 2; not 12 -- this pins the evaluation order
    st, row0, col0, n1, u, v = R.window(spec, np.array([3.0]), np.array([0.0]))
    assert (st[0], row0[0], col0[0], n1[0], u[0], v[0]) == (R.OK, 0, 0, 4, -1.0, 2.0)
    z = _one(spec, RAMP, 3.0, 0.0)["z"]
    assert z == 11.999999999999996 and z != 12.0
    assert z.hex() == "0x1.7fffffffffffep+3"


def test_basis_at_one_half():
    z = [[np.zeros(1)] * 4] * 4
    b = R.evaluate(z, np.array([0.5]), np.array([0.0]), 1.0, 1.0, R.VALUE)["b"]
    assert [float(x[0]).hex() for x in b] == ["0x1.5555555555555p-6", "0x1.eaaaaaaaaaaabp-2", "0x1.eaaaaaaaaaaabp-2", "0x1.5555555555555p-6"]


def test_constant_grid():
    block = np.full((4, 4), 6, np.float32)
    st, _, _, _, u, v = R.window(R.Spec(4, 4), np.array([1.0]), np.array([1.0]))
    assert st[0] == R.OK and u[0] == 0.0 and v[0] == 0.0
    assert _one(R.Spec(4, 4), block, 1.0, 1.0)["z"] == 6.0
    out = _one(R.Spec(4, 4, target=R.SECOND), block, 1.0, 1.0)
    assert out["zx"] == 0.0 and out["zy"] == 0.0 and list(out["normal"]) == [0.0, 0.0, 1.0]


def test_second_stage_is_not_simplified_away():
    """1.0 + u - floor(1.0 + u) loses the low bits of a small u: the model keeps the reference's two stages"""
    u = 2.0 ** -30 + 2.0 ** -80
    assert (1.0 + u) - np.floor(1.0 + u) != u
    spec = R.Spec(9, 11)
    block = np.random.default_rng(3).standard_normal((9, 11)).astype(np.float32)
    got = _one(spec, block, 4.0, 5.0 + u)["z"]
    z = [[np.array([np.float64(block[3 + r, 4 + c])]) for c in range(4)] for r in range(4)]
    two_stage = R.evaluate(z, np.array([(5.0 + u) - 4.0 - 1]), np.array([0.0]), 1.0, 1.0, R.VALUE)["z"][0]
    assert got == two_stage


def test_wrapped_windows():
    n_rows, n_cols = 6, 10
    block = np.arange(n_rows * n_cols, dtype=np.float32).reshape(n_rows, n_cols)
    for wrap, n_wrap in ((1, n_cols), (2, n_cols - 1)):
        spec = R.Spec(n_rows, n_cols, wrap=wrap)
        cols = np.array([-1.5, -0.25, 0.5, n_cols - 1.75, n_cols - 0.75, n_cols + 0.25, n_cols + 1.25, -2.5, -3.5])
        st, row0, col0, n1, u, v = R.window(spec, np.full(cols.shape, 2.5), cols)
        i_col = np.floor(cols).astype(int)
        for k in range(cols.size):
            want_col0 = n_wrap - 1 + i_col[k] if i_col[k] <= 0 else i_col[k] - 1
            want_n1 = n_wrap - want_col0
            if want_n1 < 1 or 4 - want_n1 < 1:
                assert st[k] == R.ERR_ARG, (wrap, cols[k])
                continue
            assert (st[k], row0[k], col0[k], n1[k]) == (R.OK, 1, want_col0, want_n1), (wrap, cols[k])
            assert u[k] == cols[k] - i_col[k] and v[k] == 0.5
        # the samples: n1 columns from col0, the rest from column 0
        out = R.interp(spec, block, [2.0], [-0.5])
        c0 = n_wrap - 2
        zcols = [c0 + k if k < n_wrap - c0 else k - (n_wrap - c0) for k in range(4)]
        z = [[np.array([np.float64(block[1 + r, c])]) for c in zcols] for r in range(4)]
        assert out["z"][0] == R.evaluate(z, np.array([0.5]), np.array([0.0]), 1.0, 1.0, R.VALUE)["z"][0]
        # where the reference's readBlock throws: one step further out
        assert R.interp(spec, block, [2.0, 2.0], [-3.5, n_cols + 1.5])["status"].tolist() == [R.ERR_ARG, R.ERR_ARG]
    # wrap 1: iCol == nCols is still a window (n1 = 1, n2 = 3); wrap 2: n1 = 0, rejected
    assert R.interp(R.Spec(n_rows, n_cols, wrap=1), block, [2.0], [n_cols + 0.5])["status"][0] == R.OK
    assert R.interp(R.Spec(n_rows, n_cols, wrap=2), block, [2.0], [n_cols + 0.5])["status"][0] == R.ERR_ARG
    # columns far away and infinite: Java's (int) saturates and its int arithmetic wraps; all rejected
    far = R.interp(R.Spec(n_rows, n_cols, wrap=1), block, [2.0] * 4, [1e300, -1e300, np.inf, -np.inf])
    assert far["status"].tolist() == [R.ERR_ARG] * 4


def test_fringe_edges():
    n_rows, n_cols = 7, 9
    block = np.random.default_rng(5).standard_normal((n_rows, n_cols)).astype(np.float32)
    spec = R.Spec(n_rows, n_cols)
    eps = 2.0 ** -40
    rows = [-0.5, -0.5 - eps, n_rows - 0.5, n_rows - 0.5 + eps, 3.0, 3.0, 3.0, 3.0, -np.inf, np.inf, 3.0, 3.0]
    cols = [4.0, 4.0, 4.0, 4.0, -0.5, -0.5 - eps, n_cols - 0.5, n_cols - 0.5 + eps, 4.0, 4.0, -np.inf, np.inf]
    out = R.interp(spec, block, rows, cols)
    assert out["status"].tolist() == [R.OK, R.DECLINED, R.OK, R.DECLINED] * 2 + [R.DECLINED] * 4
    assert np.isnan(out["z"][out["status"] != R.OK]).all() and not np.isnan(out["z"][out["status"] == R.OK]).any()
    # inside the fringe the coordinate is clamped onto the first / last row and column
    assert out["z"][0] == R.interp(spec, block, [0.0], [4.0])["z"][0]
    assert out["z"][2] == R.interp(spec, block, [n_rows - 1.0], [4.0])["z"][0]
    assert out["z"][4] == R.interp(spec, block, [3.0], [0.0])["z"][0]
    assert out["z"][6] == R.interp(spec, block, [3.0], [n_cols - 1.0])["z"][0]
    # a caller's wider fringe is honoured
    wide = R.Spec(n_rows, n_cols, row_fringe=(-0.5 - 2 * eps, n_rows), col_fringe=(-1.0, n_cols))
    assert R.interp(wide, block, [-0.5 - eps, 3.0], [4.0, -0.75])["status"].tolist() == [R.OK, R.OK]
    # a NaN coordinate is an argument error, whatever the other is
    assert R.interp(spec, block, [np.nan, 3.0, np.nan], [4.0, np.nan, 1e9])["status"].tolist() == [R.ERR_ARG] * 3


def test_integer_fill_reads_as_nan():
    block = np.arange(81, dtype=np.int32).reshape(9, 9) * 1000 - 7
    block[4, 4] = -99
    spec = R.Spec(9, 9, elem_type=R.INT, fill_i=-99, target=R.FIRST)
    out = R.interp(spec, block, [4.5, 7.0], [4.5, 1.5])
    assert out["status"].tolist() == [R.OK, R.OK]
    assert np.isnan(out["z"][0]) and np.isnan(out["normal"][0]).all()
    assert not np.isnan(out["z"][1]) and not np.isnan(out["normal"][1]).any()
    # (float) cell rounds an int that float32 cannot hold
    big = np.full((4, 4), 16777217, np.int32)
    assert R.samples_f32(big, R.INT, 0)[0, 0] == np.float32(16777216.0)
    short = np.full((4, 4), -32768, np.int16)
    assert np.isnan(R.samples_f32(short, R.SHORT, -32768)).all()


def test_bounds_and_spacing_statuses():
    block = np.zeros((7, 9), np.float32)
    spec = R.Spec(12, 14, block=(2, 3, 7, 9), target=R.FIRST)
    out = R.interp(spec, block, [3.5, 2.5, 3.5, 8.5, 3.5, 3.5], [4.5, 4.5, 3.5, 4.5, 10.5, 4.5], [1.0, 1.0, 1.0, 1.0, 1.0, 0.0])
    assert out["status"].tolist() == [R.OK, R.ERR_BOUNDS, R.ERR_BOUNDS, R.ERR_BOUNDS, R.ERR_BOUNDS, R.ERR_ARG]
    # a wrapped window needs column 0 in the block
    wrapped = R.Spec(12, 14, block=(2, 3, 7, 9), wrap=1)
    assert R.interp(wrapped, block, [4.5], [13.5])["status"][0] == R.ERR_BOUNDS


def test_reference_unit_test_surface():
    """InterpolationBSplineTest.testInterpolationAll restated: f = x^3 + x^2 y + y^2 x + y^3 sampled at x = j / 10, y = i / 10 on an
    11 x 11 grid, spacings 0.1, every quarter cell from 0 to 10 on both axes, the reference's own tolerances"""
    i, j = np.mgrid[0:11, 0:11].astype(np.float64)
    x, y = j / 10.0, i / 10.0
    block = (x * x * x + x * x * y + y * y * x + y * y * y).astype(np.float32)
    spec = R.Spec(11, 11, target=R.SECOND, row_spacing=0.1, col_spacing=0.1)
    q = np.arange(0, 10.25, 0.25)
    rows, cols = np.repeat(q, q.size), np.tile(q, q.size)
    out = R.interp(spec, block, rows, cols)
    assert (out["status"] == R.OK).all()
    x, y = cols / 10.0, rows / 10.0
    x2, y2 = x * x, y * y
    assert np.abs(out["z"] - (x * x2 + x2 * y + y2 * x + y * y2)).max() <= 3.0e-2
    assert np.abs(out["zx"] - (3 * x2 + 2 * x * y + y2)).max() <= 2.0e-2
    assert np.abs(out["zy"] - (x2 + 2 * x * y + 3 * y2)).max() <= 2.0e-2
    assert np.abs(out["zxx"] - (6 * x + 2 * y)).max() <= 1.0e-4
    assert np.abs(out["zyy"] - (2 * x + 6 * y)).max() <= 1.0e-4
    assert np.abs(out["zxy"] - (2 * x + 2 * y)).max() <= 1.0e-4
    assert np.abs((out["normal"] ** 2).sum(axis=1) - 1.0).max() <= 1.0e-6


def test_lattice_coordinates_are_one_product_and_one_sum():
    r, c = R.lattice_coords(0.1, -0.3, 0.7, 1.0 / 3.0, 5, 7)
    assert r.size == 35 and c.size == 35
    assert r[3 * 7 + 2] == 0.1 + 3.0 * 0.7 and c[3 * 7 + 2] == -0.3 + 2.0 * (1.0 / 3.0)
