"""CPU-only: gridfour_amd/csrc/gvrs_interp_common.h, the restatement of the reference's B-spline interpolator that the kernels
inline, compiled with g++ -O2 -ffp-contract=off (tests/csrc/interp_harness.cpp) and compared BIT FOR BIT with the numpy model of
tests/interp_ref.py: some thousand random points per target and per wrap on samples with full float32 mantissas, together with
the fixed list of points that takes every branch of the window rules; NaN where the model has NaN, every status equal."""
import numpy as np
import pytest

import interp_cases as K
import interp_ref as R

GRIDS = [((9, 11), None), ((12, 14), (2, 3, 7, 9))]


@pytest.fixture(scope="module")
def ih():
    return K.build_harness()


@pytest.mark.parametrize("wrap", [0, 1, 2])
@pytest.mark.parametrize("target", [R.VALUE, R.FIRST, R.SECOND])
def test_harness_equals_model(ih, target, wrap):
    rng = np.random.default_rng(100 + 10 * target + wrap)
    for (n_rows, n_cols), rect in GRIDS:
        # (a wrapped window needs column 0: the inner block shows ERR_BOUNDS there)
        spec = R.Spec(n_rows, n_cols, rect, R.FLOAT, wrap=wrap, target=target, row_spacing=0.37109375 + 2.0 ** -40, col_spacing=1.9 / 3.0)
        block = K.float_specials(K.random_block(rng, R.FLOAT, spec.block[2:])) if rect else K.random_block(rng, R.FLOAT, spec.block[2:])
        rows, cols = K.points(rng, spec, 3000)
        want = R.interp(spec, block, rows, cols)
        K.assert_same(K.harness_interp(ih, spec, block, rows, cols), want, (n_rows, rect))
        seen = set(want["status"].tolist())
        assert {R.OK, R.DECLINED, R.ERR_ARG} <= seen and (rect is None or R.ERR_BOUNDS in seen)
        assert not np.isnan(want["z"][want["status"] == R.OK]).all()
        # per-point column spacings, zeros among them
        cs = rng.uniform(0.25, 3.0, rows.size)
        cs[::17] = 0.0
        want = R.interp(spec, block, rows, cols, cs)
        assert target == R.VALUE or (want["status"][::17] != R.OK).all()
        K.assert_same(K.harness_interp(ih, spec, block, rows, cols, cs, threads=3), want, (n_rows, rect, "spacing"))


@pytest.mark.parametrize("elem_type,fill_i", [(R.INT, -2 ** 31), (R.INT, 12345), (R.SHORT, -32768), (R.SHORT, 0), (R.ICF, 0)])
def test_harness_equals_model_on_every_element_type(ih, elem_type, fill_i):
    rng = np.random.default_rng(200 + elem_type)
    for wrap in (0, 1):
        spec = R.Spec(9, 11, None, elem_type, fill_i, wrap=wrap, target=R.SECOND, row_spacing=30.87, col_spacing=21.5)
        block = K.random_block(rng, elem_type, (9, 11), fill_i)
        rows, cols = K.points(rng, spec, 1500)
        want = R.interp(spec, block, rows, cols)
        if elem_type != R.ICF:
            ok = want["status"] == R.OK
            assert np.isnan(want["z"][ok]).any() and not np.isnan(want["z"][ok]).all()      # fill cells read as NaN
        K.assert_same(K.harness_interp(ih, spec, block, rows, cols), want, wrap)


def test_every_window_branch_is_taken(ih):
    """the fixed list alone: standard handling, the three non-standard columns without wrap, both branches of the wrapped window
    with every n1, and each way out (NaN, row fringe, column fringe, rejected wrap)"""
    spec = R.Spec(12, 14)
    rows, cols = K.fixed_points(spec)
    st, row0, col0, n1, u, v = R.window(spec, rows, cols)
    ok = st == R.OK
    assert {0, 1, 10}.issubset(set(col0[ok].tolist())) and {0, 8}.issubset(set(row0[ok].tolist()))
    assert (u[ok] < 0).any() and (u[ok] > 1).any() and (v[ok] < 0).any() and (v[ok] > 1).any()
    for wrap, n_wrap in ((1, 14), (2, 13)):
        st, row0, col0, n1, u, v = R.window(R.Spec(12, 14, wrap=wrap), rows, cols)
        ok = st == R.OK
        assert {1, 2, 3, 4} == set(n1[ok].tolist()) and (st == R.ERR_ARG).any()
        i_col = np.floor(cols[ok & (n1 < 4)])
        assert (i_col <= 0).any() and (i_col > 0).any()
